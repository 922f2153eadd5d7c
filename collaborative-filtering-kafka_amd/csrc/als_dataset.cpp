// als_dataset.cpp -- host data layer (include/als_host.h), first of three units (als_dataset_impl.h names the others):
// dataset lifetime, Netflix-format ingest, datasets from rating triples, and the plain queries.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "als_dataset_impl.h"

using namespace cfk_detail;

namespace {

void finalize(als_dataset* ds) {
    const int64_t n = (int64_t)ds->rating.size();
    for (int s = 0; s < 2; ++s) {
        const std::vector<int32_t>& raw = s == 0 ? ds->movie : ds->user;
        int32_t mx = 0;
        for (int32_t v : raw) mx = std::max(mx, v);
        // counting presence over [0, max] (ids are bounded by int32 and were checked >= 0)
        std::vector<int32_t> rank((size_t)mx + 1, -1);
        for (int32_t v : raw) rank[v] = 0;
        ds->ids[s].clear();
        for (int64_t v = 0; v <= mx; ++v)
            if (rank[v] == 0) {
                rank[v] = (int32_t)ds->ids[s].size();
                ds->ids[s].push_back(v);
            }
        ds->dense[s].resize(n);
        for (int64_t t = 0; t < n; ++t) ds->dense[s][t] = rank[raw[t]];
    }
}

// BufferedReader.readLine semantics: a line ends at "\n", "\r" or "\r\n" and may be of any length
// (NetflixDataFormatProducer.java:44); the file is streamed through a fixed buffer.
struct LineReader {
    FILE* f;
    std::vector<char> buf = std::vector<char>(1 << 20);
    size_t pos = 0, len = 0;
    bool eof = false;
    bool refill() {   // false, and nothing read, once the file has ended
        if (eof) return false;
        len = fread(buf.data(), 1, buf.size(), f);
        pos = 0;
        eof = len == 0;
        return !eof;
    }
    bool next(std::string& out) {
        out.clear();
        bool any = false;
        for (;;) {
            if (pos == len && !refill()) return any;
            any = true;
            const char* b = buf.data() + pos;
            const char* e = buf.data() + len;
            const char* p = b;
            while (p < e && *p != '\n' && *p != '\r') ++p;
            out.append(b, p);
            pos += (size_t)(p - b);
            if (p == e) continue;                        // line continues in the next buffer
            const char term = *p;
            ++pos;
            if (term == '\r') {                          // "\r\n" counts as one terminator
                if (pos == len) refill();
                if (pos < len && buf[pos] == '\n') ++pos;
            }
            return true;
        }
    }
};

// Integer.parseInt / Short.parseShort: optional sign, decimal digits only
bool parse_int(const char* b, const char* e, int64_t& v) {
    if (b == e) return false;
    bool neg = false;
    if (*b == '-' || *b == '+') {
        neg = *b == '-';
        ++b;
        if (b == e) return false;
    }
    int64_t x = 0;
    for (; b < e; ++b) {
        if (*b < '0' || *b > '9') return false;
        x = x * 10 + (*b - '0');
        if (x > (int64_t)1 << 40) return false;
    }
    v = neg ? -x : x;
    return true;
}

}  // namespace

extern "C" {

int als_dataset_load_netflix(const char* path, als_dataset** out) {
    if (!path || !out) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    std::unique_ptr<FILE, int (*)(FILE*)> f(fopen(path, "rb"), fclose);
    if (!f) return fail(ALS_ERR_IO, "cannot open %s", path);
    std::unique_ptr<als_dataset> ds(new als_dataset());
    LineReader lines{f.get()};
    std::string line;
    int64_t current = -1, lineno = 0;
    while (lines.next(line)) {
        ++lineno;
        const size_t n = line.size();
        const char* b = line.data();
        const char* e = b + n;
        if (n > 0 && b[n - 1] == ':') {                                   // row.endsWith(":")
            const char* colon = (const char*)memchr(b, ':', n);           // row.split(":")[0]
            int64_t v;
            if (!parse_int(b, colon, v) || v < 0 || v > INT32_MAX)
                return fail(ALS_ERR_PARSE, "%s:%lld: bad movie header", path, (long long)lineno);
            current = v;
            continue;
        }
        const char* c1 = (const char*)memchr(b, ',', n);
        const char* c2 = c1 ? (const char*)memchr(c1 + 1, ',', e - c1 - 1) : nullptr;
        const char* rend = c2 ? c2 : e;
        int64_t uid, r;
        if (!c1 || !parse_int(b, c1, uid) || !parse_int(c1 + 1, rend, r) || uid < 0 || uid > INT32_MAX ||
            r < -32768 || r > 32767)
            return fail(ALS_ERR_PARSE, "%s:%lld: expected UserID,Rating,Date", path, (long long)lineno);
        if (current < 0)
            return fail(ALS_ERR_PARSE, "%s:%lld: rating before the first movie header", path, (long long)lineno);
        ds->movie.push_back((int32_t)current);
        ds->user.push_back((int32_t)uid);
        ds->rating.push_back((int16_t)r);
    }
    finalize(ds.get());
    *out = ds.release();
    return ALS_OK;
}

int als_dataset_from_ratings(int64_t n, const int32_t* movie_ids, const int32_t* user_ids, const int16_t* ratings,
                             als_dataset** out) {
    if (!out || n < 0 || (n > 0 && (!movie_ids || !user_ids || !ratings)))
        return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    *out = nullptr;
    for (int64_t t = 0; t < n; ++t)
        if (movie_ids[t] < 0 || user_ids[t] < 0)
            return fail(ALS_ERR_INVALID_ARGUMENT, "negative id at rating %lld", (long long)t);
    std::unique_ptr<als_dataset> ds(new als_dataset());
    ds->movie.assign(movie_ids, movie_ids + n);
    ds->user.assign(user_ids, user_ids + n);
    ds->rating.assign(ratings, ratings + n);
    finalize(ds.get());
    *out = ds.release();
    return ALS_OK;
}

int als_dataset_destroy(als_dataset* ds) {
    delete ds;
    return ALS_OK;
}

int als_dataset_counts(const als_dataset* ds, int64_t* n_movies, int64_t* n_users, int64_t* nnz) {
    if (!ds) return fail(ALS_ERR_INVALID_ARGUMENT, "dataset is NULL");
    if (n_movies) *n_movies = (int64_t)ds->ids[0].size();
    if (n_users) *n_users = (int64_t)ds->ids[1].size();
    if (nnz) *nnz = (int64_t)ds->rating.size();
    return ALS_OK;
}

int als_dataset_ids(const als_dataset* ds, int side, int64_t* ids) {
    if (!ds || !check_side(side) || !ids) return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    std::copy(ds->ids[side].begin(), ds->ids[side].end(), ids);
    return ALS_OK;
}

int als_dataset_ratings(const als_dataset* ds, int32_t* movie_ids, int32_t* user_ids, int16_t* ratings) {
    if (!ds) return fail(ALS_ERR_INVALID_ARGUMENT, "dataset is NULL");
    if (movie_ids) std::copy(ds->movie.begin(), ds->movie.end(), movie_ids);
    if (user_ids) std::copy(ds->user.begin(), ds->user.end(), user_ids);
    if (ratings) std::copy(ds->rating.begin(), ds->rating.end(), ratings);
    return ALS_OK;
}

int als_dataset_count_duplicates(const als_dataset* ds, int64_t* n_dup) {
    if (!ds || !n_dup) return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    const int64_t n = (int64_t)ds->rating.size();
    std::vector<uint64_t> key(n);
    for (int64_t t = 0; t < n; ++t) key[t] = ((uint64_t)(uint32_t)ds->dense[1][t] << 32) | (uint32_t)ds->dense[0][t];
    std::sort(key.begin(), key.end());
    int64_t d = 0;
    for (int64_t t = 1; t < n; ++t) d += key[t] == key[t - 1];
    *n_dup = d;
    return ALS_OK;
}

}  // extern "C"
