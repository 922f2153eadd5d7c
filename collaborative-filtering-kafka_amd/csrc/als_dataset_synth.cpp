// als_dataset_synth.cpp -- host data layer, the seeded synthetic generators: user degrees, item popularity and its alias
// table, one deterministic rating list per user, and the drivers that keep every rating or one shard's, movie-major.
#include <atomic>
#include <cmath>
#include <memory>
#include <numeric>
#include <thread>

#include "als_dataset_impl.h"

using namespace cfk_detail;

namespace {

// Shape of a synthetic rating matrix: log-normal user activity (mu, sigma of the log, per-user cap; scaled to
// exactly nnz) and item popularity w(rank) over a seeded random rank order.
struct SynthSpec {
    double mu, sigma;
    int64_t cap;
    double rank_offset, exponent;     // w(rank) = (rank + 1 + rank_offset)^-exponent
    uint64_t perm_salt;
};

// user degrees log-normal (median 96, mean 208.2 at Netflix scale, cap 17,653); movies (rank + 320)^-1.85
SynthSpec netflix_spec() {
    return {std::log(96.0), std::sqrt(2.0 * std::log(208.2 / 96.0)), 17653, 320.0, 1.85, 0x30F1EULL};
}

// user activity log-normal with sigma 1.5 and mean nnz / n_users; item popularity ~ rank^-1 (Zipf);
// per-user cap n_items / 10 (the heaviest users and items are the load-balance stress)
SynthSpec powerlaw_spec(int64_t n_users, int64_t n_items, int64_t nnz) {
    const double sigma = 1.5, mean = (double)nnz / (double)std::max<int64_t>(1, n_users);
    return {std::log(mean) - 0.5 * sigma * sigma, sigma, std::max<int64_t>(1, n_items / 10), 0.0, 1.0, 0x9A11ULL};
}

// Ratings per user: log-normal draws scaled to nnz, each within [1, cap], the total exactly nnz.
std::vector<int64_t> user_degrees(const SynthSpec& sp, int64_t cap, int64_t n_users, int64_t nnz, uint64_t seed) {
    std::vector<int64_t> deg(n_users);
    Rng rng(mix64(seed ^ 0xDE6DE6ULL));
    std::vector<double> raw(n_users);
    double sum = 0;
    for (int64_t u = 0; u < n_users; ++u) {
        // Box-Muller
        double u1 = rng.uniform(), u2 = rng.uniform();
        if (u1 < 1e-300) u1 = 1e-300;
        const double z = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
        raw[u] = std::exp(sp.mu + sp.sigma * z);
        sum += raw[u];
    }
    const double scale = (double)nnz / sum;
    int64_t tot = 0;
    for (int64_t u = 0; u < n_users; ++u) {
        deg[u] = std::min<int64_t>(cap, std::max<int64_t>(1, (int64_t)std::llround(raw[u] * scale)));
        tot += deg[u];
    }
    // exact total: adjust random users one rating at a time
    while (tot != nnz) {
        const int64_t u = (int64_t)rng.below(n_users);
        if (tot < nnz && deg[u] < cap) { ++deg[u]; ++tot; }
        else if (tot > nnz && deg[u] > 1) { --deg[u]; --tot; }
    }
    return deg;
}

// Item popularity: w(rank) = (rank + 1 + offset)^-exponent over a seeded random rank order.
std::vector<double> popularity(const SynthSpec& sp, int64_t n_movies, uint64_t seed) {
    std::vector<double> w(n_movies);
    std::vector<int32_t> perm(n_movies);
    std::iota(perm.begin(), perm.end(), 0);
    Rng rng(mix64(seed ^ sp.perm_salt));
    for (int64_t i = n_movies - 1; i > 0; --i) std::swap(perm[i], perm[rng.below(i + 1)]);
    for (int64_t r = 0; r < n_movies; ++r) w[perm[r]] = std::pow((double)(r + 1) + sp.rank_offset, -sp.exponent);
    return w;
}

// Alias table (Vose) over the weights w: item i with probability prob[i], else alias[i], after a uniform i.
struct AliasTable {
    std::vector<double> prob;
    std::vector<int32_t> alias;
    explicit AliasTable(const std::vector<double>& w) : prob(w.size()), alias(w.size()) {
        const int64_t n = (int64_t)w.size();
        const double tw = std::accumulate(w.begin(), w.end(), 0.0);
        std::vector<double> p(n);
        std::vector<int32_t> small, large;
        for (int64_t i = 0; i < n; ++i) {
            p[i] = w[i] * (double)n / tw;
            (p[i] < 1.0 ? small : large).push_back((int32_t)i);
        }
        while (!small.empty() && !large.empty()) {
            const int32_t s = small.back(), l = large.back();
            small.pop_back();
            prob[s] = p[s];
            alias[s] = l;
            p[l] = (p[l] + p[s]) - 1.0;
            if (p[l] < 1.0) {
                large.pop_back();
                small.push_back(l);
            }
        }
        for (int32_t i : large) { prob[i] = 1.0; alias[i] = i; }
        for (int32_t i : small) { prob[i] = 1.0; alias[i] = i; }
    }
};

// One user's distinct movies (sorted, 0-based) and ratings: a function of the seed and the user alone, whichever
// thread draws it. dst and rat take deg[u] entries; stamp is the calling thread's own, n_movies entries from -1.
struct UserSampler {
    uint64_t seed;
    int64_t n_users, n_movies;
    std::vector<int64_t> deg;
    AliasTable table;
    void operator()(int64_t u, int32_t* dst, int16_t* rat, std::vector<int32_t>& stamp) const {
        // rating histogram of data_sample_medium.txt: 1: 4.55%, 2: 9.78%, 3: 28.37%, 4: 33.51%, 5: 23.80%
        const double cdf[5] = {0.0455, 0.0455 + 0.0978, 0.0455 + 0.0978 + 0.2837, 0.0455 + 0.0978 + 0.2837 + 0.3351, 1.0};
        Rng rng(mix64(seed * 0x9E3779B97F4A7C15ULL + (uint64_t)u));
        const int64_t d = deg[u];
        int64_t got = 0, tries = 0;
        const int64_t max_tries = 64 * d + 100000;
        while (got < d && tries < max_tries) {
            ++tries;
            const int64_t i = (int64_t)rng.below(n_movies);
            const int32_t m = rng.uniform() < table.prob[i] ? (int32_t)i : table.alias[i];
            if (stamp[m] == (int32_t)u) continue;
            stamp[m] = (int32_t)u;
            dst[got++] = m;
        }
        for (int64_t m = (int64_t)rng.below(n_movies); got < d; m = (m + 1) % n_movies)   // fallback
            if (stamp[m] != (int32_t)u) {
                stamp[m] = (int32_t)u;
                dst[got++] = (int32_t)m;
            }
        std::sort(dst, dst + d);
        for (int64_t t = 0; t < d; ++t) {
            const double x = rng.uniform();
            int r = 0;
            while (r < 4 && x >= cdf[r]) ++r;
            rat[t] = (int16_t)(r + 1);
        }
    }
};

// The worker pool: nthreads threads take ranges of 256 users until none is left. Thread w calls make_worker(w) once
// and what that returns with each range [u0, u1) it takes; what a thread keeps between ranges (its stamps) lives there.
template <class MakeWorker>
void for_user_ranges(int64_t n_users, int nthreads, MakeWorker make_worker) {
    std::atomic<int64_t> next_user{0};
    std::vector<std::thread> pool;
    for (int w = 0; w < nthreads; ++w)
        pool.emplace_back([&, w] {
            auto range = make_worker(w);
            for (int64_t u0; (u0 = next_user.fetch_add(256)) < n_users;) range(u0, std::min<int64_t>(n_users, u0 + 256));
        });
    for (auto& t : pool) t.join();
}

// Movie-major arrival order (users ascending inside a movie): a stable counting sort by movie of the kept ratings.
// visit(f) calls f(movie, user, rating), 0-based, for every kept rating in user-major order; it runs twice.
template <class Visit>
void movie_major(als_dataset* ds, int64_t n_movies, Visit visit) {
    std::vector<int64_t> pos(n_movies + 1, 0);   // counts, shifted by one, then each movie's next place
    visit([&](int32_t m, int32_t, int16_t) { ++pos[m + 1]; });
    for (int64_t m = 0; m < n_movies; ++m) pos[m + 1] += pos[m];
    const int64_t kept = pos[n_movies];
    ds->movie.resize(kept);
    ds->user.resize(kept);
    ds->rating.resize(kept);
    visit([&](int32_t m, int32_t u, int16_t r) {
        const int64_t p = pos[m]++;
        ds->movie[p] = m + 1;
        ds->user[p] = u + 1;
        ds->rating[p] = r;
    });
}

// Dense ranks are known directly: ids are 1..n and every entity is rated.
void identity_ids(als_dataset* ds, int64_t n_users, int64_t n_movies) {
    const int64_t kept = (int64_t)ds->rating.size();
    ds->ids[0].resize(n_movies);
    ds->ids[1].resize(n_users);
    std::iota(ds->ids[0].begin(), ds->ids[0].end(), 1);
    std::iota(ds->ids[1].begin(), ds->ids[1].end(), 1);
    ds->dense[0].resize(kept);
    ds->dense[1].resize(kept);
    for (int64_t t = 0; t < kept; ++t) {
        ds->dense[0][t] = ds->movie[t] - 1;
        ds->dense[1][t] = ds->user[t] - 1;
    }
}

// Every movie rated at least once: re-point one entry of a popular movie (keeps nnz exact). um: the user-major movie
// lists, user u's at [uoff[u], uoff[u + 1]), each sorted.
void rate_every_movie(std::vector<int32_t>& um, const std::vector<int64_t>& uoff, int64_t n_movies, uint64_t seed) {
    const int64_t nnz = (int64_t)um.size();
    std::vector<int64_t> mdeg(n_movies, 0);
    for (int64_t t = 0; t < nnz; ++t) ++mdeg[um[t]];
    Rng rng(mix64(seed ^ 0xF111ULL));
    for (int64_t m = 0; m < n_movies; ++m) {
        if (mdeg[m] > 0) continue;
        for (;;) {
            const int64_t t = (int64_t)rng.below(nnz);
            if (mdeg[um[t]] < 2) continue;
            // owning user of entry t
            const int64_t u = (int64_t)(std::upper_bound(uoff.begin(), uoff.end(), t) - uoff.begin()) - 1;
            int32_t *b = um.data() + uoff[u], *e = um.data() + uoff[u + 1];
            if (std::binary_search(b, e, (int32_t)m)) continue;
            --mdeg[um[t]];
            um[t] = (int32_t)m;
            ++mdeg[m];
            std::sort(b, e);   // keep the row sorted (ratings stay iid)
            break;
        }
    }
}

// The whole matrix: per-user lists side by side (user-major), the every-movie-rated pass, one placement pass.
int generate_full(const UserSampler& sample, int nthreads, als_dataset* ds) {
    const int64_t n_users = sample.n_users, n_movies = sample.n_movies;
    std::vector<int64_t> uoff(n_users + 1, 0);
    for (int64_t u = 0; u < n_users; ++u) uoff[u + 1] = uoff[u] + sample.deg[u];
    std::vector<int32_t> um(uoff[n_users]);
    std::vector<int16_t> ur(uoff[n_users]);
    for_user_ranges(n_users, nthreads, [&](int) {
        return [&, stamp = std::vector<int32_t>(n_movies, -1)](int64_t u0, int64_t u1) mutable {
            for (int64_t u = u0; u < u1; ++u) sample(u, um.data() + uoff[u], ur.data() + uoff[u], stamp);
        };
    });
    rate_every_movie(um, uoff, n_movies, sample.seed);
    movie_major(ds, n_movies, [&](auto place) {
        for (int64_t u = 0; u < n_users; ++u)
            for (int64_t t = uoff[u]; t < uoff[u + 1]; ++t) place(um[t], (int32_t)u, ur[t]);
    });
    return ALS_OK;
}

// Shard-restricted: every user's list is generated (the same draws as above), only shard `keep`'s ratings are kept
// (movie id % G == keep or user id % G == keep, the in-blocks of both sides of that shard: about 2/G of nnz per process),
// in the full dataset's relative arrival order, plus every user's rating sum (U0) and the movie degrees (the
// every-movie-rated guarantee, which the full path enforces with a global fix-up pass: the restricted path requires
// that no movie is unrated, true of every configured shape: the rarest configs[4] item expects ~140 ratings).
int generate_restricted(const UserSampler& sample, int nthreads, int G, int keep, als_dataset* ds) {
    const int64_t n_users = sample.n_users, n_movies = sample.n_movies;
    struct Kept { int32_t m, u; int16_t r; };
    std::vector<std::vector<Kept>> kept((n_users + 255) / 256);   // per range of 256 users, user-major
    std::vector<std::vector<int64_t>> mdeg_t(nthreads);
    ds->user_sum.assign(n_users, 0);
    ds->user_cnt.assign(n_users, 0);
    for_user_ranges(n_users, nthreads, [&](int w) {
        mdeg_t[w].assign(n_movies, 0);
        return [&, &mdeg = mdeg_t[w], stamp = std::vector<int32_t>(n_movies, -1), lst = std::vector<int32_t>(),
                rat = std::vector<int16_t>()](int64_t u0, int64_t u1) mutable {
            std::vector<Kept>& mine = kept[u0 / 256];
            for (int64_t u = u0; u < u1; ++u) {
                const int64_t d = sample.deg[u];
                lst.resize(d);
                rat.resize(d);
                sample(u, lst.data(), rat.data(), stamp);
                const bool own_user = (u + 1) % G == keep;
                int64_t sum = 0;
                for (int64_t t = 0; t < d; ++t) {
                    ++mdeg[lst[t]];
                    sum += rat[t];
                    if (own_user || (lst[t] + 1) % G == keep) mine.push_back({lst[t], (int32_t)u, rat[t]});
                }
                ds->user_sum[u] = sum;
                ds->user_cnt[u] = d;
            }
        };
    });
    for (int64_t m = 0; m < n_movies; ++m) {
        int64_t d = 0;
        for (auto& v : mdeg_t) d += v[m];
        if (d == 0)
            return fail(ALS_ERR_UNSUPPORTED, "movie %lld unrated: the shard-restricted generator needs every "
                        "movie rated (use the full generator)", (long long)m + 1);
    }
    mdeg_t.clear();
    movie_major(ds, n_movies, [&](auto place) {
        for (const auto& range : kept)
            for (const Kept& k : range) place(k.m, k.u, k.r);
    });
    return ALS_OK;
}

// G > 1: the shard-restricted dataset of shard `keep`.
int synthesize(const SynthSpec& sp, int64_t n_users, int64_t n_movies, int64_t nnz, uint64_t seed, int nthreads,
               als_dataset** out, int G = 1, int keep = 0) {
    if (!out) return fail(ALS_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (G < 1 || keep < 0 || keep >= G) return fail(ALS_ERR_INVALID_ARGUMENT, "bad shard %d of %d", keep, G);
    if (n_users < 1 || n_movies < 1 || n_users > INT32_MAX - 1 || n_movies > INT32_MAX - 1)
        return fail(ALS_ERR_INVALID_ARGUMENT, "bad entity counts");
    if (nnz < std::max(n_users, n_movies) || nnz > n_users * n_movies / 2)
        return fail(ALS_ERR_INVALID_ARGUMENT, "nnz must be in [max(n_users, n_movies), n_users*n_movies/2]");
    if (nthreads <= 0) nthreads = (int)std::max(1u, std::thread::hardware_concurrency());
    nthreads = std::min(nthreads, 64);
    const int64_t cap = std::min<int64_t>(sp.cap, n_movies);
    if (cap * n_users < nnz) return fail(ALS_ERR_INVALID_ARGUMENT, "nnz exceeds n_users * per-user cap");
    const UserSampler sample{seed, n_users, n_movies, user_degrees(sp, cap, n_users, nnz, seed),
                             AliasTable(popularity(sp, n_movies, seed))};
    std::unique_ptr<als_dataset> ds(new als_dataset());
    const int rc = G > 1 ? generate_restricted(sample, nthreads, G, keep, ds.get()) : generate_full(sample, nthreads, ds.get());
    if (rc != ALS_OK) return rc;
    identity_ids(ds.get(), n_users, n_movies);
    *out = ds.release();
    return ALS_OK;
}

}  // namespace

extern "C" {

int als_dataset_synthetic_netflix(int64_t n_users, int64_t n_movies, int64_t nnz, uint64_t seed, int nthreads,
                                  als_dataset** out) {
    return synthesize(netflix_spec(), n_users, n_movies, nnz, seed, nthreads, out);
}

int als_dataset_synthetic_powerlaw(int64_t n_users, int64_t n_items, int64_t nnz, uint64_t seed, int nthreads,
                                   als_dataset** out) {
    return synthesize(powerlaw_spec(n_users, n_items, nnz), n_users, n_items, nnz, seed, nthreads, out);
}

int als_dataset_synthetic_powerlaw_shard(int64_t n_users, int64_t n_items, int64_t nnz, uint64_t seed, int nthreads,
                                         int n_shards, int shard, als_dataset** out) {
    return synthesize(powerlaw_spec(n_users, n_items, nnz), n_users, n_items, nnz, seed, nthreads, out, n_shards, shard);
}

int als_dataset_synthetic_netflix_shard(int64_t n_users, int64_t n_movies, int64_t nnz, uint64_t seed, int nthreads,
                                        int n_shards, int shard, als_dataset** out) {
    return synthesize(netflix_spec(), n_users, n_movies, nnz, seed, nthreads, out, n_shards, shard);
}

}  // extern "C"
