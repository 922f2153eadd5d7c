// Private to als_foldin.hip and als_implicit.hip: the one kernel that solves a query's k x k system from its entries,
// for both models, and its launch glue. Include inside namespace cfk { namespace {, after als_fold_tiles.h.
//
// als_fold_solve_kernel<T, KP, Args>: Args = FoldinArgs solves the explicit normal equation of als_foldin.hip,
// Args = ImplicitArgs the implicit-feedback one of als_implicit.hip. One 256-thread workgroup owns one whole query
// (grid-stride over the queries), so a query's bits depend on nothing but its own entries (and, implicit, on G, lambda
// and alpha): no atomics, no split across workgroups, every sum in one fixed order.
//   gather : batches of the query's opposite rows go into LDS through q_idx, 16 bytes per lane, a row's loads
//            contiguous; the tail of the last batch is zero-filled up to a whole MFMA step (4 entries). The next batch
//            is loaded into registers while the Gram of the current one runs.
//   Gram   : lower-triangle 16 x 16 tiles on the matrix pipe at full input precision (v_mfma_f32_16x16x4_f32 /
//            v_mfma_f64_16x16x4_f64: a k-ordered fma chain per element). The tiles are dealt over the 4 waves (tile t to
//            wave t % 4) and stay in accumulator registers over all batches. Per 4 entries a wave reads one operand
//            register per 16-feature block it needs -- lane (g, c) holds Y[entry 4 s + g][16 b + c], which is both the A
//            operand of tile row b and the B operand of tile column b -- and issues all its tiles.
//   RHS    : on the VALU, thread f < KP owns feature f, entries in order.
//   solve  : the tiles go through LDS into a thread-per-element layout; the regulariser on the k true diagonal entries,
//            Jacobi scaling, a right-looking Cholesky in registers over the k true features (the padded ones are an
//            identity block that nothing couples to; one barrier per column, the pivot column broadcast through LDS),
//            forward and backward substitution with the vector in registers (one barrier per step). fp64 adds the one
//            refinement step of als_solve_generic, the residual formed from the rows themselves.
// The model is chosen by `if constexpr (IMPLICIT)` at five places, each commented there: the query index, the per-batch
// right-hand side and Gram step, + G, the regulariser, and the refinement's residual. Everything else is one text.
// KP is the engine's factor stride: 16, 32, 64 or 128, and in fp64 also 80, 96 and 112 (65..112 features are on the
// generic solve path there, whose stride is the next multiple of 16): fold_by_kp.
// DESIGN.md sections 3.9 and 3.10 have the layout, the resource figures and the measurements.
#pragma once

// fold_gram_batch with a per-entry weight: tile (I, J) += (w y[I])^T y[J], w_e = alpha tb[e] (tb: the batch's ratings;
// lane (g, c) of step s holds entry 4 s + g, so one weight per lane and step).
template <class T, int KP, int W, int MT>
__device__ __forceinline__ void implicit_gram_batch(typename FoldAcc<T>::type (&acc)[MT], const T* __restrict__ stage,
                                                    const T* __restrict__ tb, T alpha, int nsteps, int lane) {
    constexpr int C = KP / 16, NT = foldin_tiles(KP), P = foldin_pitch(KP);
    const T* p = stage + (lane >> 4) * P + (lane & 15);
    const T* wr = tb + (lane >> 4);
    for (int s = 0; s < nsteps; ++s, p += 4 * P, wr += 4) {
        T op[C], wop[C];
        const T w = alpha * wr[0];
        static_for<0, C>([&](auto b) {
            op[b] = p[16 * b];
            wop[b] = w * op[b];
        });
        static_for<0, NT>([&](auto t) {
            constexpr int tt = decltype(t)::value;
            if constexpr (tt % 4 == W) {
                constexpr int I = fold_tile_row(tt), J = fold_tile_col(tt);
                acc[tt / 4] = fold_mfma(wop[I], op[J], acc[tt / 4]);
            }
        });
    }
}

// The queries, the tables and lambda of either model's arguments.
__host__ __device__ inline const FoldinArgs& fold_queries(const FoldinArgs& a) { return a; }
__host__ __device__ inline const FoldinArgs& fold_queries(const ImplicitArgs& a) { return a.f; }

template <class T, int KP, class Args>
__global__ __launch_bounds__(FOLDIN_THREADS) void als_fold_solve_kernel(Args args, int batch) {
    constexpr int C = KP / 16, NT = foldin_tiles(KP), MT = (NT + 3) / 4, P = foldin_pitch(KP);
    constexpr bool REFINE = std::is_same<T, double>::value;
    constexpr bool IMPLICIT = std::is_same<Args, ImplicitArgs>::value;
    typedef typename FoldAcc<T>::type Acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
    T* G = (T*)fsm;                               // [NT][16][FOLDIN_TILE_PITCH]
    T* stage = G + NT * FOLDIN_TILE_ELEMS;        // [batch][P]
    T* scl = stage + batch * P;                   // [KP] Jacobi scale 1 / sqrt(a_ii)
    T* dg = scl + KP;                             // [KP] diagonal of L
    T* bc = dg + KP;                              // [KP] substitution: the component being broadcast
    T* xs = bc + KP;                              // [KP] solution (refinement)
    T* tb = xs + KP;                              // [batch] ratings, then per-entry residuals
    const FoldinArgs& a = fold_queries(args);
    const int tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
    const int ke = a.k;
    const T* opp = (const T*)a.opp;
    const T* Gt = nullptr;   // implicit: the opposite table's Gram [KP][KP], and w_e = alpha r_e
    T alpha = T(0);
    if constexpr (IMPLICIT) {
        Gt = (const T*)args.gram;
        alpha = (T)args.alpha;
    }

    // v <- (L L^T)^-1 v for the vector held one component per thread (tid < ke)
    auto chol_solve = [&](T v) -> T {
        for (int j = 0; j < ke; ++j) {   // forward: L y = v
            if (tid == j) bc[j] = v / dg[j];
            __syncthreads();
            if (tid > j && tid < ke) v -= G[fold_at(tid, j)] * bc[j];
        }
        T y = tid < ke ? bc[tid] : T(0);
        __syncthreads();
        for (int j = ke - 1; j >= 0; --j) {   // backward: L^T x = y
            if (tid == j) bc[j] = y / dg[j];
            __syncthreads();
            if (tid < j) y -= G[fold_at(j, tid)] * bc[j];
        }
        const T x = tid < ke ? bc[tid] : T(0);
        __syncthreads();
        return x;
    };

    for (int64_t qi = blockIdx.x; qi < a.n_queries; qi += gridDim.x) {
        // Query index. Implicit walks a host-made permutation, longest query first (a training half has rows of 200k
        // entries next to rows of 1); a query's bits do not depend on it.
        int64_t q = qi;
        if constexpr (IMPLICIT) q = args.order[qi];
        const int64_t lo = a.q_ptr[q];
        const int n = (int)(a.q_ptr[q + 1] - lo);
        T* out = (T*)a.out + q * KP;
        T* dst = a.dst_rows ? (T*)a.self + a.dst_rows[q] * KP : nullptr;
        if (n == 0) {   // b = 0 (cannot occur in the reference): the zero vector, written directly. Workgroup-uniform.
            if (tid < KP) {
                out[tid] = T(0);
                if (dst) dst[tid] = T(0);
            }
            continue;
        }
        const int32_t* idx = a.q_idx + lo;
        const int16_t* rat = a.q_rat + lo;

        Acc acc[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = Acc{};
        T rhs = T(0);
        FoldBatch<T, KP> fb;
        fold_load<T, KP>(fb, opp, idx, rat, min(batch, n), tid);
        for (int base = 0; base < n; base += batch) {
            const int nb = min(batch, n - base), nb4 = (nb + 3) & ~3;
            fold_store<T, KP>(fb, stage, tb, nb4, tid);
            __syncthreads();
            if (base + batch < n)   // the next batch's rows travel while this one is multiplied
                fold_load<T, KP>(fb, opp, idx + base + batch, rat + base + batch, min(batch, n - base - batch), tid);
            // Per-batch right-hand side and Gram step. Explicit: Y^T r and Y^T Y. Implicit: sum (1 + w_e) y_e over the
            // entries with r_e > 0, and tile (I, J) accumulates mfma(w y[I], y[J]) -- a second operand register set,
            // one multiply per feature block and MFMA step. Only the lower triangle is read afterwards, so the diagonal
            // tiles need not be bitwise symmetric.
            if constexpr (IMPLICIT) {
                if (tid < KP)
                    for (int e = 0; e < nb; ++e) {
                        const T r = tb[e];
                        if (r > T(0)) rhs += (T(1) + alpha * r) * stage[e * P + tid];
                    }
                FOLD_BY_WAVE(wave, implicit_gram_batch, acc, stage, tb, alpha, nb4 >> 2, lane)
            } else {
                if (tid < KP)
                    for (int e = 0; e < nb; ++e) rhs += tb[e] * stage[e * P + tid];
                FOLD_BY_WAVE(wave, fold_gram_batch, acc, stage, nb4 >> 2, lane)
            }
            __syncthreads();
        }
        FOLD_BY_WAVE(wave, fold_store_tiles, acc, G, lane, FoldTilePitch<FOLDIN_TILE_PITCH>{})
        __syncthreads();

        // thread (ty, tx) owns element (ty, tx) of every tile, here and in the factorisation below
        const int ty = tid >> 4, tx = tid & 15;
        const int own = ty * FOLDIN_TILE_PITCH + tx;
        // + G. Implicit: every thread adds the matching elements of the table's Gram from global memory.
        if constexpr (IMPLICIT) {
            static_for<0, NT>([&](auto t) {
                constexpr int tt = decltype(t)::value;
                G[tt * FOLDIN_TILE_ELEMS + own] += Gt[(16 * fold_tile_row(tt) + ty) * KP + 16 * fold_tile_col(tt) + tx];
            });
            __syncthreads();
        }
        // Regulariser on the true features: lambda (float) n of the explicit model (MFeatureCalculator.java:91-95), the
        // plain lambda of the implicit one. Then D^-1/2 A D^-1/2.
        T reg;
        if constexpr (IMPLICIT) reg = (T)a.lambda;
        else reg = (T)a.lambda * (T)n;
        if (tid < KP) {
            T s = T(1);
            if (tid < ke) {
                const T d = G[fold_at(tid, tid)] + reg;
                G[fold_at(tid, tid)] = d;
                s = T(1) / sqrt(d);
            }
            scl[tid] = s;
        }
        __syncthreads();
        // Right-looking Cholesky in registers: thread (ty, tx) holds its element of every tile, scaled as it is loaded.
        // Column j = 16 J + jj: its owners (tx = jj) publish the unscaled column, pivot included, through LDS (two
        // buffers in turn, one barrier per column); every thread scales the entries of its rows and columns by
        // 1 / sqrt(pivot) itself, the owners keep theirs as L, and the trailing tiles take the rank-1 update. J is a
        // compile-time index, so no register array is indexed dynamically. Rows above the diagonal of a diagonal tile
        // hold values nobody reads.
        T g[NT];
        static_for<0, NT>([&](auto t) {
            constexpr int tt = decltype(t)::value;
            g[tt] = G[tt * FOLDIN_TILE_ELEMS + own] * scl[16 * fold_tile_row(tt) + ty] * scl[16 * fold_tile_col(tt) + tx];
        });
        static_for<0, C>([&](auto Jc) {
            constexpr int J = decltype(Jc)::value;
            for (int jj = 0; jj < 16; ++jj) {
                const int j = 16 * J + jj;
                if (j < ke) {   // workgroup-uniform
                    T* cb = (j & 1) ? xs : bc;
                    if (tx == jj) static_for<J, C>([&](auto ac) {
                        constexpr int A = decltype(ac)::value;
                        cb[16 * A + ty] = g[A * (A + 1) / 2 + J];
                    });
                    __syncthreads();
                    const T piv = cb[j];
                    const T rinv = T(1) / sqrt(piv);
                    if (tid == 0) dg[j] = sqrt(piv);
                    T li[C], ll[C];
                    static_for<J, C>([&](auto ac) {
                        constexpr int A = decltype(ac)::value;
                        li[A] = cb[16 * A + ty] * rinv;
                        ll[A] = cb[16 * A + tx] * rinv;
                    });
                    static_for<J, C>([&](auto ac) {
                        constexpr int A = decltype(ac)::value;
                        // tile (A, J): the column itself where tx = jj, the finished columns left of it stay
                        T& gj = g[A * (A + 1) / 2 + J];
                        gj = tx == jj ? li[A] : (tx > jj ? gj - li[A] * ll[J] : gj);
                        static_for<J + 1, A + 1>([&](auto bc_) {
                            constexpr int B = decltype(bc_)::value;
                            g[A * (A + 1) / 2 + B] -= li[A] * ll[B];
                        });
                    });
                }
            }
        });
        __syncthreads();   // the last column's readers are done with bc / xs, which the substitution reuses
        static_for<0, NT>([&](auto t) {
            constexpr int tt = decltype(t)::value;
            G[tt * FOLDIN_TILE_ELEMS + own] = g[tt];
        });
        __syncthreads();
        T x = chol_solve(rhs * (tid < KP ? scl[tid] : T(0)));
        x *= tid < KP ? scl[tid] : T(0);
        if constexpr (REFINE) {
            // one step of iterative refinement, x += A^-1 (b - A x), the residual from the rows themselves (the triangle
            // now holds L). Explicit: b - A x = sum_e y_e (r_e - y_e . x) - lambda n x. Implicit:
            // sum_e y_e [(r_e > 0)(1 + w_e) - w_e (y_e . x)] - G x - lambda x; G is symmetric, so row tid of G x reads
            // column tid: consecutive threads, consecutive addresses.
            if (tid < KP) xs[tid] = x;
            T res = -reg * x;
            __syncthreads();
            if constexpr (IMPLICIT) {
                if (tid < KP)
                    for (int j = 0; j < ke; ++j) res -= Gt[j * KP + tid] * xs[j];
            }
            for (int base = 0; base < n; base += batch) {
                const int nb = min(batch, n - base), nb4 = (nb + 3) & ~3;
                fold_load<T, KP>(fb, opp, idx + base, rat + base, nb, tid);
                fold_store<T, KP>(fb, stage, tb, nb4, tid);
                __syncthreads();
                for (int e = wave; e < nb; e += 4) {   // the residual coefficient t_e of entry e, one wave per entry
                    T d = T(0);
                    for (int f = lane; f < KP; f += 64) d += stage[e * P + f] * xs[f];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
                    if (lane == 0) {
                        if constexpr (IMPLICIT) {   // t_e = (r_e > 0)(1 + w_e) - w_e (y_e . x)
                            const T r = tb[e], w = alpha * r;
                            tb[e] = (r > T(0) ? T(1) + w : T(0)) - w * d;
                        } else {   // t_e = r_e - y_e . x
                            tb[e] -= d;
                        }
                    }
                }
                __syncthreads();
                if (tid < KP)
                    for (int e = 0; e < nb; ++e) res += stage[e * P + tid] * tb[e];
                __syncthreads();
            }
            const T dx = chol_solve(res * (tid < KP ? scl[tid] : T(0)));
            x += dx * (tid < KP ? scl[tid] : T(0));
        }
        if (tid < KP) {
            const T v = tid < ke ? x : T(0);
            out[tid] = v;
            if (dst) dst[tid] = v;
        }
        __syncthreads();
    }
}

// ---- launch glue -----------------------------------------------------------------------------------------------------

// f(std::integral_constant<int, KP>) for the stride kp of an engine of element type T: 16, 32, 64, 128, and in fp64 also
// 80, 96, 112 (engines of 65..112 features are on the generic solve path, whose stride is the next multiple of 16).
template <class T, class F>
hipError_t fold_by_kp(int kp, F&& f) {
    switch (kp) {
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        default: break;
    }
    if constexpr (std::is_same<T, double>::value) {
        switch (kp) {
            case 80: return f(std::integral_constant<int, 80>{});
            case 96: return f(std::integral_constant<int, 96>{});
            case 112: return f(std::integral_constant<int, 112>{});
            default: break;
        }
    }
    return hipErrorInvalidValue;
}

// The launch of either model is served by this plan: the geometry of foldin_plan, the LDS of the kernel's carve-up.
inline bool fold_plan_ok(int precision, int kp, const FoldinArgs& a, const FoldinPlan& plan) {
    const int elem = precision == 0 ? 4 : 8;
    return kp <= FOLDIN_MAX_KP && a.k >= 1 && a.k <= kp && plan.threads == FOLDIN_THREADS && plan.grid >= 1 &&
           plan.grid <= a.n_queries && plan.grid <= INT32_MAX && plan.batch >= 4 && plan.batch % 4 == 0 &&
           plan.batch <= FOLDIN_MAX_BATCH && plan.lds_bytes == foldin_lds_bytes(kp, elem, plan.batch) &&
           plan.lds_bytes <= FOLDIN_LDS_LIMIT;
}

template <class T, class Args>
hipError_t launch_fold_solve(int kp, const Args& a, const FoldinPlan& plan, hipStream_t s) {
    return fold_by_kp<T>(kp, [&](auto kpc) {
        constexpr int KP = decltype(kpc)::value;
        // the fp64 k = 128 shape needs more than the 64 KiB a kernel gets by default. Every call sets the same bound per
        // instantiation (its plan does not depend on the call), so engines of several devices and host threads cannot
        // lower it under one another's launch.
        hipError_t e = hipFuncSetAttribute((const void*)als_fold_solve_kernel<T, KP, Args>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes);
        if (e != hipSuccess) return e;
        als_fold_solve_kernel<T, KP, Args><<<(unsigned)plan.grid, FOLDIN_THREADS, (size_t)plan.lds_bytes, s>>>(a, plan.batch);
        return hipGetLastError();
    });
}
