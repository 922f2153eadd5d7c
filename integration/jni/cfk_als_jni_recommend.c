/*
 * cfk_als_jni_recommend.c -- the native behind AlsNative.recommend (als_recommend, include/als.h). Part of
 * cfk_als_jni.c, which includes it at its end: it uses that file's static helpers (ENGINE, fail_status, fail_arg,
 * alloc_n) and is built into the same libcfk_als_jni.so by the same command.
 *
 * AlsNative.recommend is a public Java method that checks the array lengths and calls the private native recommend0;
 * the public natives of AlsNative are the set that tests/test_jni_shim.py pins and tests/test_integration_java.py
 * pairs with the JNIEXPORT functions of cfk_als_jni.c, so this one, which is not among them, has its file and its
 * own source-level check (tests/test_recommend_host.py) and runs through the mock JVM in tests/test_gpu_recommend.py.
 *
 * Same rules as predict: the arrays are copied with Get<Type>ArrayRegion into native buffers, the lengths are checked
 * here too (IllegalArgumentException naming the array, before any C ABI call), and no critical region is held while
 * als_recommend waits on the GPU. The scores go back with SetFloatArrayRegion; the positions are copied into outIdx
 * in a critical region around one memcpy, entered only after als_recommend has returned.
 */
#include <string.h>

JNIEXPORT void JNICALL Java_de_hpi_collaborativefilteringkafka_nativeals_AlsNative_recommend0(
        JNIEnv* env, jclass cls, jlong engine, jlongArray user_rows, jlongArray movie_rows, jint top_n,
        jlongArray excl_ptr, jintArray excl_idx, jintArray out_idx, jfloatArray out_score) {
    (void)cls;
    if ((excl_ptr == NULL) != (excl_idx == NULL)) {
        fail_arg(env, "recommend: exclPtr and exclIdx must both be given or both be null");
        return;
    }
    const jsize nu = (*env)->GetArrayLength(env, user_rows), nm = (*env)->GetArrayLength(env, movie_rows);
    const int64_t cells = (int64_t)nu * (int64_t)(top_n > 0 ? top_n : 0);
    if ((int64_t)(*env)->GetArrayLength(env, out_idx) != cells) {
        fail_arg(env, "recommend: outIdx.length must be userRows.length * topN");
        return;
    }
    if ((int64_t)(*env)->GetArrayLength(env, out_score) != cells) {
        fail_arg(env, "recommend: outScore.length must be userRows.length * topN");
        return;
    }
    const jsize np = excl_ptr ? (*env)->GetArrayLength(env, excl_ptr) : 0;
    const jsize ne = excl_idx ? (*env)->GetArrayLength(env, excl_idx) : 0;
    if (excl_ptr && (int64_t)np != (int64_t)nu + 1) {
        fail_arg(env, "recommend: exclPtr.length must be userRows.length + 1");
        return;
    }
    jlong* u = alloc_n(env, nu, sizeof(jlong), "recommend: userRows");
    jlong* m = u ? alloc_n(env, nm, sizeof(jlong), "recommend: movieRows") : NULL;
    jlong* ep = m ? alloc_n(env, np, sizeof(jlong), "recommend: exclPtr") : NULL;
    jint* ei = ep ? alloc_n(env, ne, sizeof(jint), "recommend: exclIdx") : NULL;
    jint* idx = ei ? alloc_n(env, (jsize)cells, sizeof(jint), "recommend: outIdx") : NULL;
    jfloat* score = idx ? alloc_n(env, (jsize)cells, sizeof(jfloat), "recommend: outScore") : NULL;
    if (score != NULL) {
        (*env)->GetLongArrayRegion(env, user_rows, 0, nu, u);
        (*env)->GetLongArrayRegion(env, movie_rows, 0, nm, m);
        if (excl_ptr) {
            (*env)->GetLongArrayRegion(env, excl_ptr, 0, np, ep);
            (*env)->GetIntArrayRegion(env, excl_idx, 0, ne, ei);
        }
        if (!(*env)->ExceptionCheck(env)) {
            /* the C ABI cannot see exclIdx.length: the ranges must lie inside the array */
            if (excl_ptr && (ep[0] < 0 || ep[nu] > (jlong)ne)) {
                fail_arg(env, "recommend: exclPtr points outside exclIdx");
            } else if (!fail_status(env, "als_recommend",
                                    als_recommend(ENGINE(engine), (const int64_t*)u, nu, (const int64_t*)m, nm, top_n,
                                                  excl_ptr ? (const int64_t*)ep : NULL,
                                                  excl_ptr ? (const int32_t*)ei : NULL, (int32_t*)idx, score)) &&
                       nu > 0 && nm > 0) {   /* nothing to do: als_recommend leaves the outputs untouched */
                (*env)->SetFloatArrayRegion(env, out_score, 0, (jsize)cells, score);
                void* dst = (*env)->GetPrimitiveArrayCritical(env, out_idx, NULL);
                if (dst != NULL) {
                    memcpy(dst, idx, (size_t)cells * sizeof(jint));
                    (*env)->ReleasePrimitiveArrayCritical(env, out_idx, dst, 0);
                }
            }
        }
    }
    free(score);
    free(idx);
    free(ei);
    free(ep);
    free(m);
    free(u);
}
