// Stand-alone check of the host data layer (include/als_host.h): the synthetic generators, the shard and slot
// geometry, U0, the Netflix-format loader and the CSV writers. tests/test_dataset_host.py compiles this file with the
// data-layer sources under -fsanitize=address,undefined (and, for the synthesis cases, -fsanitize=thread) and runs it
// as its own process. It prints one JSON line per case; tests/golden/dataset_digests.json pins every line.
//
//   dataset_check DIR            every case (input and output files are written under DIR)
//   dataset_check DIR synth      the synthesis cases only (the multi-threaded code)
//   dataset_check DIR time_full | time_shard [digest]
//                                one generation at a tenth of the Netflix shape, 16 threads: wall seconds
//
// Digests are FNV-1a 64 over the raw bytes of each array, chained in the order given.
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "als.h"
#include "als_host.h"

namespace {

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t n) {
        const unsigned char* c = (const unsigned char*)p;
        for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
    }
    template <class T>
    void val(T v) { bytes(&v, sizeof(T)); }
    template <class T>
    void vec(const std::vector<T>& v) {
        if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
    }
    std::string hex() const {
        char b[17];
        snprintf(b, sizeof b, "%016llx", (unsigned long long)h);
        return b;
    }
};

// One JSON line, printed when the case goes out of scope.
struct Case {
    std::string line;
    explicit Case(const std::string& name) { line = "{\"case\": \"" + name + "\""; }
    ~Case() { printf("%s}\n", line.c_str()); }
    static std::string quoted(const std::string& s) {
        std::string q = "\"";
        for (char c : s) {
            if (c == '"' || c == '\\') q.push_back('\\');
            q.push_back(c);
        }
        return q + "\"";
    }
    void raw(const char* key, const std::string& v) { line += std::string(", \"") + key + "\": " + v; }
    void num(const char* key, long long v) { raw(key, std::to_string(v)); }
    void flag(const char* key, bool v) { raw(key, v ? "true" : "false"); }
    void str(const char* key, const std::string& v) { raw(key, quoted(v)); }
    void digest(const char* key, const Fnv& f) { str(key, f.hex()); }
    void list(const char* key, const std::vector<std::string>& v) {
        std::string s = "[";
        for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + quoted(v[i]);
        raw(key, s + "]");
    }
    // status and, on failure, the message
    void status(int st) {
        num("status", st);
        if (st != ALS_OK) str("error", als_last_error());
    }
};

struct Triples {
    std::vector<int32_t> movie, user;
    std::vector<int16_t> rating;
    bool operator==(const Triples& o) const { return movie == o.movie && user == o.user && rating == o.rating; }
    void push(int32_t m, int32_t u, int16_t r) {
        movie.push_back(m);
        user.push_back(u);
        rating.push_back(r);
    }
    Fnv fnv() const {
        Fnv f;
        f.vec(movie);
        f.vec(user);
        f.vec(rating);
        return f;
    }
};

struct Dataset {   // owns an als_dataset
    als_dataset* ds = nullptr;
    Dataset() = default;
    Dataset(const Dataset&) = delete;
    Dataset& operator=(const Dataset&) = delete;
    ~Dataset() { als_dataset_destroy(ds); }
    int64_t count(int what) const {   // 0 movies, 1 users, 2 ratings
        int64_t c[3] = {0, 0, 0};
        als_dataset_counts(ds, &c[0], &c[1], &c[2]);
        return c[what];
    }
    Triples triples() const {
        Triples t;
        const int64_t n = count(2);
        t.movie.resize(n);
        t.user.resize(n);
        t.rating.resize(n);
        als_dataset_ratings(ds, t.movie.data(), t.user.data(), t.rating.data());
        return t;
    }
};

using Full = int (*)(int64_t, int64_t, int64_t, uint64_t, int, als_dataset**);
using Shard = int (*)(int64_t, int64_t, int64_t, uint64_t, int, int, int, als_dataset**);
struct Generator {
    const char* name;
    Full full;
    Shard shard;
};
const Generator GENERATORS[2] = {
    {"netflix", als_dataset_synthetic_netflix, als_dataset_synthetic_netflix_shard},
    {"powerlaw", als_dataset_synthetic_powerlaw, als_dataset_synthetic_powerlaw_shard},
};
const uint64_t SEED = 5;

// ---------------------------------------------------------------- synthesis

void synthesis_cases() {
    const int64_t nu = 2000, nm = 300, nnz = 40000;
    for (const Generator& g : GENERATORS) {
        Triples full;
        for (int nthreads : {1, 3}) {
            Case c(std::string("synth_") + g.name + "_t" + std::to_string(nthreads));
            Dataset d;
            const int st = g.full(nu, nm, nnz, SEED, nthreads, &d.ds);
            c.status(st);
            if (st != ALS_OK) continue;
            full = d.triples();
            c.num("kept", d.count(2));
            c.num("n_movies", d.count(0));
            c.num("n_users", d.count(1));
            c.digest("digest", full.fnv());
        }
        for (int shard = 0; shard < 3; ++shard) {
            Case c(std::string("synth_") + g.name + "_g3_s" + std::to_string(shard));
            Dataset d;
            const int st = g.shard(nu, nm, nnz, SEED, 3, 3, shard, &d.ds);
            c.status(st);
            if (st != ALS_OK) continue;
            const Triples got = d.triples();
            Triples want;   // the full dataset's ratings of this shard's in-blocks, in order
            for (size_t t = 0; t < full.rating.size(); ++t)
                if (full.movie[t] % 3 == shard || full.user[t] % 3 == shard)
                    want.push(full.movie[t], full.user[t], full.rating[t]);
            c.num("kept", d.count(2));
            c.num("n_movies", d.count(0));
            c.num("n_users", d.count(1));
            c.digest("digest", got.fnv());
            c.flag("equals_full_filtered", got == want);
        }
    }
}

void fixup_cases() {
    // more movies than the generated lists reach: the every-movie-rated pass re-points ratings
    const int64_t nu = 300, nm = 2000, nnz = 3000;
    for (const Generator& g : GENERATORS) {
        Case c(std::string("fixup_") + g.name);
        Dataset d;
        const int st = g.full(nu, nm, nnz, SEED, 3, &d.ds);
        c.status(st);
        if (st != ALS_OK) continue;
        const Triples t = d.triples();
        std::vector<int64_t> deg(nm + 1, 0);
        for (int32_t m : t.movie) ++deg[m];
        int64_t once = 0, never = 0;
        for (int64_t m = 1; m <= nm; ++m) {
            once += deg[m] == 1;
            never += deg[m] == 0;
        }
        int64_t dup = -1;
        als_dataset_count_duplicates(d.ds, &dup);
        c.num("kept", d.count(2));
        c.num("movies_rated_once", once);
        c.num("movies_unrated", never);
        c.num("duplicates", dup);
        c.digest("digest", t.fnv());
    }
    Case c("fixup_netflix_shard_g2_s1");
    Dataset d;
    c.status(als_dataset_synthetic_netflix_shard(nu, nm, nnz, SEED, 3, 2, 1, &d.ds));
    c.flag("out_is_null", d.ds == nullptr);
}

void synthesis_argument_cases() {
    {
        Case c("synth_arg_cap");
        Dataset d;
        c.status(als_dataset_synthetic_powerlaw(40, 60, 1200, SEED, 1, &d.ds));
    }
    {
        Case c("synth_arg_nnz_low");
        Dataset d;
        c.status(als_dataset_synthetic_netflix(100, 50, 99, SEED, 1, &d.ds));
    }
    {
        Case c("synth_arg_nnz_high");
        Dataset d;
        c.status(als_dataset_synthetic_netflix(100, 50, 2501, SEED, 1, &d.ds));
    }
    {
        Case c("synth_arg_counts");
        Dataset d;
        c.status(als_dataset_synthetic_powerlaw(0, 50, 100, SEED, 1, &d.ds));
    }
    {
        Case c("synth_arg_shard");
        Dataset d;
        c.status(als_dataset_synthetic_netflix_shard(2000, 300, 40000, SEED, 1, 3, 3, &d.ds));
    }
    {
        Case c("synth_arg_shard_negative");
        Dataset d;
        c.status(als_dataset_synthetic_powerlaw_shard(2000, 300, 40000, SEED, 1, 3, -1, &d.ds));
    }
    {
        Case c("synth_arg_out_null");
        c.status(als_dataset_synthetic_netflix(2000, 300, 40000, SEED, 1, nullptr));
    }
    {
        Case c("synth_shard_arg_out_null");
        c.status(als_dataset_synthetic_powerlaw_shard(2000, 300, 40000, SEED, 1, 3, 0, nullptr));
    }
}

// ---------------------------------------------------------------- shard geometry and U0

Fnv u0_digest(const als_dataset* ds, int G, int* status) {
    int64_t n_slots = 0;
    als_dataset_shard_info(ds, 1, G, 0, nullptr, nullptr, nullptr, nullptr, &n_slots);
    const int k = 5, ld = 6;
    std::vector<float> out((size_t)(n_slots + 1) * ld, -1.f);   // one row more than needed: zeroed too
    *status = als_dataset_init_user_factors(ds, k, 42, G, out.data(), ld, n_slots + 1);
    Fnv f;
    f.vec(out);
    return f;
}

// shard_block (row_ptr, col_idx, ratings, row_ids) and shard_coo (rows, cols, ratings) of one shard
void block_digests(const als_dataset* ds, int side, int G, int shard, Fnv& block, Fnv& coo, bool& ok) {
    int64_t n_rows = 0, nnz = 0;
    ok = als_dataset_shard_info(ds, side, G, shard, &n_rows, nullptr, &nnz, nullptr, nullptr) == ALS_OK && ok;
    std::vector<int64_t> row_ptr(n_rows + 1), row_ids(n_rows);
    std::vector<int32_t> col(nnz), rows(nnz), cols(nnz);
    std::vector<int16_t> rat(nnz), crat(nnz);
    ok = als_dataset_shard_block(ds, side, G, shard, row_ptr.data(), col.data(), rat.data(), row_ids.data()) == ALS_OK && ok;
    ok = als_dataset_shard_coo(ds, side, G, shard, rows.data(), cols.data(), crat.data()) == ALS_OK && ok;
    ok = ok && row_ptr[n_rows] == nnz;
    block.vec(row_ptr);
    block.vec(col);
    block.vec(rat);
    block.vec(row_ids);
    coo.vec(rows);
    coo.vec(cols);
    coo.vec(crat);
}

void geometry_of(const std::string& name, als_dataset* ds) {
    for (int G : {1, 3})
        for (int C : {1, 2}) {
            Case c("geom_" + name + "_g" + std::to_string(G) + "_c" + std::to_string(C));
            bool ok = als_dataset_set_slot_chunks(ds, 1, C) == ALS_OK;
            Fnv info, layout, slots;
            std::vector<std::string> block, coo;
            for (int side = 0; side < 2; ++side) {
                for (int shard = 0; shard < G; ++shard) {
                    int64_t v[5] = {-1, -1, -1, -1, -1};
                    ok = als_dataset_shard_info(ds, side, G, shard, &v[0], &v[1], &v[2], &v[3], &v[4]) == ALS_OK && ok;
                    info.bytes(v, sizeof v);
                    Fnv b, o;
                    block_digests(ds, side, G, shard, b, o, ok);
                    block.push_back(b.hex());
                    coo.push_back(o.hex());
                }
                int64_t sc = -1;
                int nc = -1;
                ok = als_dataset_slot_layout(ds, side, G, &sc, &nc) == ALS_OK && ok;
                layout.val(sc);
                layout.val(nc);
                int64_t n = 0;
                als_dataset_counts(ds, side == 0 ? &n : nullptr, side == 1 ? &n : nullptr, nullptr);
                std::vector<int64_t> slot_of(n, -1), ids(n, -1);
                ok = als_dataset_slots(ds, side, G, slot_of.data()) == ALS_OK && ok;
                ok = als_dataset_ids(ds, side, ids.data()) == ALS_OK && ok;
                slots.vec(slot_of);
                slots.vec(ids);
            }
            int st = 0;
            const Fnv u0 = u0_digest(ds, G, &st);
            c.flag("ok", ok && st == ALS_OK);
            c.digest("shard_info", info);
            c.digest("slot_layout", layout);
            c.digest("slots", slots);
            c.list("shard_block", block);   // movie side shards 0..G-1, then user side
            c.list("shard_coo", coo);
            c.digest("u0", u0);
        }
    als_dataset_set_slot_chunks(ds, 1, 1);
}

void geometry_cases() {
    Dataset net;
    als_dataset_synthetic_netflix(2000, 300, 40000, SEED, 3, &net.ds);
    geometry_of("netflix", net.ds);

    // gaps in the ids of both sides, id 0, ids that share a shard under G = 3, one pair rated twice
    const int32_t m[] = {7, 7, 0, 12, 3, 7, 12, 100, 3, 0, 41, 41, 7, 12, 100, 3, 9, 9, 41, 0,
                         7, 100, 12, 3, 41, 9, 0, 7, 12, 41, 3};
    const int32_t u[] = {5, 11, 5, 2, 30, 2, 11, 5, 5, 64, 2, 30, 64, 30, 11, 2, 5, 17, 17, 17,
                         17, 64, 5, 64, 5, 11, 2, 5, 64, 11, 17};
    const int16_t r[] = {5, 3, 4, 1, 2, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 1, 2, 3, 4, 5, 5, 4, 2, 2, 1, 3};
    const int64_t n = (int64_t)(sizeof r / sizeof r[0]);
    Dataset small;
    als_dataset_from_ratings(n, m, u, r, &small.ds);
    geometry_of("small", small.ds);

    for (auto* d : {&net, &small}) {
        Case c(d == &net ? "duplicates_netflix" : "duplicates_small");
        int64_t dup = -1;
        c.status(als_dataset_count_duplicates(d->ds, &dup));
        c.num("duplicates", dup);
        c.num("n_movies", d->count(0));
        c.num("n_users", d->count(1));
        c.num("nnz", d->count(2));
    }
    {
        // the restricted dataset answers its own shard's queries, and U0, as the full one does
        Case c("restricted_netflix_g3_s1");
        Dataset d;
        c.status(als_dataset_synthetic_netflix_shard(2000, 300, 40000, SEED, 3, 3, 1, &d.ds));
        bool ok = true;
        std::vector<std::string> block, coo;
        for (int side = 0; side < 2; ++side) {
            Fnv b, o;
            block_digests(d.ds, side, 3, 1, b, o, ok);
            block.push_back(b.hex());
            coo.push_back(o.hex());
        }
        int st = 0;
        const Fnv u0 = u0_digest(d.ds, 3, &st);
        c.flag("ok", ok && st == ALS_OK);
        c.list("shard_block", block);   // shard 1 of the movie side, of the user side
        c.list("shard_coo", coo);
        c.digest("u0", u0);
    }
    int64_t buf[64];
    int32_t ibuf[64];
    int16_t sbuf[64];
    float fbuf[64];
    als_dataset* ds = small.ds;
    { Case c("geom_arg_side"); c.status(als_dataset_shard_info(ds, 2, 1, 0, buf, buf, buf, buf, buf)); }
    { Case c("geom_arg_side_negative"); c.status(als_dataset_slots(ds, -1, 1, buf)); }
    { Case c("geom_arg_shard"); c.status(als_dataset_shard_block(ds, 0, 3, 3, buf, ibuf, sbuf, buf)); }
    { Case c("geom_arg_shard_info_shard"); c.status(als_dataset_shard_info(ds, 0, 3, -1, buf, buf, buf, buf, buf)); }
    { Case c("geom_arg_row_ptr_null"); c.status(als_dataset_shard_block(ds, 0, 1, 0, nullptr, ibuf, sbuf, buf)); }
    { Case c("geom_arg_coo_null"); c.status(als_dataset_shard_coo(ds, 1, 1, 0, ibuf, nullptr, sbuf)); }
    { Case c("geom_arg_coo_shard"); c.status(als_dataset_shard_coo(ds, 1, 2, 2, ibuf, ibuf, sbuf)); }
    { Case c("geom_arg_n_shards"); c.status(als_dataset_slot_layout(ds, 0, 0, buf, nullptr)); }
    { Case c("geom_arg_chunks"); c.status(als_dataset_set_slot_chunks(ds, 1, 0)); }
    { Case c("geom_arg_chunks_side"); c.status(als_dataset_set_slot_chunks(ds, 3, 1)); }
    { Case c("geom_arg_ids_side"); c.status(als_dataset_ids(ds, 2, buf)); }
    { Case c("geom_arg_dataset_null"); c.status(als_dataset_counts(nullptr, buf, buf, buf)); }
    { Case c("geom_arg_ratings_null"); c.status(als_dataset_ratings(nullptr, ibuf, ibuf, sbuf)); }
    { Case c("geom_arg_duplicates_null"); c.status(als_dataset_count_duplicates(ds, nullptr)); }
    { Case c("u0_arg_ld"); c.status(als_dataset_init_user_factors(ds, 5, 42, 1, fbuf, 4, 16)); }
    { Case c("u0_arg_rows"); c.status(als_dataset_init_user_factors(ds, 5, 42, 1, fbuf, 5, 2)); }
    { Case c("from_ratings_arg_negative"); als_dataset* o = nullptr; const int32_t neg[] = {1, -2}; c.status(als_dataset_from_ratings(2, neg, neg, sbuf, &o)); }
    { Case c("from_ratings_arg_null"); als_dataset* o = nullptr; c.status(als_dataset_from_ratings(2, nullptr, ibuf, sbuf, &o)); }
    {
        Case c("u01");
        Fnv f;
        for (int64_t id : {0ll, 1ll, 17770ll, 2649429ll})
            for (int feat = 1; feat < 4; ++feat) f.val(als_u01(42, id, feat));
        c.digest("digest", f);
    }
}

// ---------------------------------------------------------------- loader

const size_t BUF = 1 << 20;   // the reader's buffer

bool write_file(const char* name, const std::string& content) {
    FILE* f = fopen(name, "wb");
    if (!f) return false;
    const bool ok = fwrite(content.data(), 1, content.size(), f) == content.size();
    return fclose(f) == 0 && ok;
}

void load_case(const char* name, const std::string& content, const Triples& want) {
    Case c(std::string("load_") + name);
    const std::string file = std::string(name) + ".txt";
    if (!write_file(file.c_str(), content)) {
        c.str("error", "cannot write the input file");
        return;
    }
    Dataset d;
    const int st = als_dataset_load_netflix(file.c_str(), &d.ds);
    c.status(st);
    c.num("bytes", (long long)content.size());
    if (st != ALS_OK) {
        c.flag("out_is_null", d.ds == nullptr);
        return;
    }
    const Triples got = d.triples();
    c.num("n", (long long)got.rating.size());
    c.flag("matches", got == want);
    c.digest("digest", got.fnv());
}

// "1:\n7,3,xxxx...": a header and one rating line whose ignored date field pads the file to `size` bytes
std::string padded_to(size_t size) {
    std::string s = "1:\n7,3,";
    s.append(size - s.size(), 'x');
    return s;
}

void loader_cases() {
    Triples two;
    two.push(1, 7, 3);
    two.push(1, 8, 4);
    // "\r" is the last byte of the first buffer, "\n" the first of the second: one terminator
    load_case("crlf_across_buffers", padded_to(BUF - 1) + "\r\n8,4,2005-01-01\n", two);
    // a lone "\r" as the last byte of a buffer, the next line starts the next buffer
    load_case("cr_ends_buffer", padded_to(BUF - 1) + "\r8,4,2005-01-01\n", two);
    {
        // "\r" ends the buffer and the file
        Triples one;
        one.push(1, 7, 3);
        load_case("cr_ends_buffer_and_file", padded_to(BUF - 1) + "\r", one);
    }
    {
        // user id 123456: "123" ends the first buffer, "456" starts the second
        Triples t;
        t.push(1, 7, 3);
        t.push(1, 123456, 5);
        load_case("user_id_across_buffers", padded_to(BUF - 4) + "\n123456,5,2005-01-01\n", t);
    }
    {
        // a line of two and a half buffers, then a short one
        Triples t;
        t.push(1, 7, 3);
        t.push(2, 10, 2);
        load_case("line_longer_than_buffer", padded_to(2 * BUF + BUF / 2) + "\n2:\n10,2,z\n", t);
    }
    {
        Triples t;
        t.push(3, 5, 4);
        t.push(3, 6, 2);
        load_case("no_final_terminator", "3:\n5,4,2005-09-06\n6,2,2005-09-07", t);
    }
    {
        // every terminator, blank-free; a header with text after the id's colon still ends with ":"
        Triples t;
        t.push(4, 1, 1);
        t.push(4, 2, -2);
        t.push(17, 3, 32767);
        t.push(17, 2649429, 5);
        load_case("mixed_terminators", "4:\r\n1,1,a\r2,-2\n17:x:\r\n3,+32767,b,c\n2649429,5,d\r\n", t);
    }
    load_case("empty_file", "", Triples());
    // errors: the message names the file and the line, "\r\n" counting once
    load_case("err_bad_header", "1:\r\n5,3,d\r\nabc:\r\n6,3,d\r\n", Triples());
    load_case("err_header_out_of_range", "2147483648:\n", Triples());
    load_case("err_rating_before_header", "5,3,2005-01-01\n1:\n", Triples());
    load_case("err_not_a_rating_line", "1:\r5,3,d\r\nnot-a-rating-line\n", Triples());
    load_case("err_rating_40000", "1:\n5,3,d\n6,40000,d\n", Triples());
    load_case("err_blank_line", "1:\n5,3,d\n\n6,4,d\n", Triples());
    {
        Case c("load_err_missing_file");
        Dataset d;
        c.status(als_dataset_load_netflix("missing.txt", &d.ds));
    }
    {
        Case c("load_err_null");
        Dataset d;
        c.status(als_dataset_load_netflix(nullptr, &d.ds));
    }
}

// ---------------------------------------------------------------- CSV

void file_result(Case& c, int st, const char* name) {
    c.status(st);
    if (st != ALS_OK) return;
    Fnv f;
    long long size = -1;
    if (FILE* in = fopen(name, "rb")) {
        char buf[4096];
        size = 0;
        for (size_t n; (n = fread(buf, 1, sizeof buf, in)) > 0; size += (long long)n) f.bytes(buf, n);
        fclose(in);
    }
    c.num("bytes", size);
    c.digest("digest", f);
}

void csv_cases() {
    const float inf = std::numeric_limits<float>::infinity();
    // both layouts of Double.toString and its specials; 1e-40f is a float denormal
    const float v[12] = {std::nanf(""), inf, -inf, -0.0f, 0.001f, 9999999.f, 1.0e7f, 1.0e-4f, 1e-40f, -123.456f, 42.f, 0.f};
    {
        Case c("csv_prediction_matrix");
        file_result(c, als_write_prediction_matrix_csv("matrix.csv", v, 3, 4), "matrix.csv");
    }
    {
        // P = U M^T with exact products: rows 1 x, 0.5 x, -3 x of the values (-3 x rounds once), leading dimensions
        // wider than k
        const int k = 2;
        const float U[3 * 3] = {1.f, 0.f, 99.f, 0.5f, 0.25f, 99.f, -3.f, 0.001f, 99.f};
        const float M[4 * 4] = {0.001f, 0.f, 99.f, 99.f, 9999999.f, 0.f, 99.f, 99.f,
                                1e-40f, 0.f, 99.f, 99.f, 42.f, 8.f, 99.f, 99.f};
        Case c("csv_prediction");
        file_result(c, als_write_prediction_csv("prediction.csv", U, 3, 3, M, 4, 4, k), "prediction.csv");
    }
    {
        Case c("csv_prediction_specials");   // k = 1, U = 1: the matrix case's values through the dot product
        const float one[3] = {1.f, 1.f, 1.f};
        file_result(c, als_write_prediction_csv("specials.csv", one, 3, 1, v, 4, 1, 1), "specials.csv");
    }
    {
        Case c("csv_prediction_empty");
        file_result(c, als_write_prediction_matrix_csv("empty.csv", nullptr, 0, 4), "empty.csv");
    }
    const int64_t users[3] = {10, 2649429, 30};
    const int64_t movies[12] = {5, -1, 17770, 1, -1, -1, -1, -1, 0, 3, -1, 9};
    {
        Case c("csv_recommendations");   // padding entries (movie id < 0) are left out; user 2649429 has none
        file_result(c, als_write_recommendations_csv("recommend.csv", users, 3, 4, movies, v), "recommend.csv");
    }
    { Case c("csv_err_prediction_path"); c.status(als_write_prediction_csv("no_such_dir/p.csv", v, 3, 1, v, 4, 1, 1)); }
    { Case c("csv_err_matrix_path"); c.status(als_write_prediction_matrix_csv("no_such_dir/m.csv", v, 3, 4)); }
    { Case c("csv_err_recommendations_path"); c.status(als_write_recommendations_csv("no_such_dir/r.csv", users, 3, 4, movies, v)); }
    { Case c("csv_arg_prediction"); c.status(als_write_prediction_csv("x.csv", v, 3, 1, v, 4, 1, 2)); }
    { Case c("csv_arg_matrix"); c.status(als_write_prediction_matrix_csv("x.csv", nullptr, 3, 4)); }
    { Case c("csv_arg_recommendations"); c.status(als_write_recommendations_csv("x.csv", users, 3, 0, movies, v)); }
}

// ---------------------------------------------------------------- generator timing

int time_generator(bool shard, bool digest) {
    const auto t0 = std::chrono::steady_clock::now();
    Dataset d;
    const int st = shard ? als_dataset_synthetic_netflix_shard(48019, 17770, 10000000, 0xA15, 16, 8, 0, &d.ds)
                         : als_dataset_synthetic_netflix(48019, 17770, 10000000, 0xA15, 16, &d.ds);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (st != ALS_OK) {
        fprintf(stderr, "%s\n", als_last_error());
        return 1;
    }
    // the digest copies the ratings out, so it is left out where the peak memory of the generator is measured
    printf("{\"case\": \"%s\", \"seconds\": %.4f, \"kept\": %lld, \"digest\": \"%s\"}\n", shard ? "time_shard" : "time_full", s,
           (long long)d.count(2), digest ? d.triples().fnv().hex().c_str() : "");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2 || chdir(argv[1]) != 0) {   // relative file names: the messages that name a file stay the same
        fprintf(stderr, "usage: dataset_check SCRATCH_DIR [synth | time_full | time_shard [digest]]\n");
        return 2;
    }
    const std::string mode = argc > 2 ? argv[2] : "";
    if (mode == "time_full" || mode == "time_shard") return time_generator(mode == "time_shard", argc > 3);
    synthesis_cases();
    fixup_cases();
    if (mode == "synth") return 0;
    synthesis_argument_cases();
    geometry_cases();
    loader_cases();
    csv_cases();
    return 0;
}
