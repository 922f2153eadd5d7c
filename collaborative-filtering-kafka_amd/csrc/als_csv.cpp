// als_csv.cpp -- host data layer, text output (include/als_host.h): the collector's prediction CSV and the top-N
// lists, their values printed as Java's Double.toString prints them.
#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "als_error.h"
#include "als_host.h"

using namespace cfk_detail;

namespace {

// Java Double.toString layout over the shortest round-trip digits.
std::string java_double(double v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "Infinity" : "-Infinity";
    if (v == 0.0) return std::signbit(v) ? "-0.0" : "0.0";
    char buf[64];
    auto res = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::scientific);
    std::string s(buf, res.ptr);
    std::string sign;
    if (s[0] == '-') {
        sign = "-";
        s = s.substr(1);
    }
    const size_t epos = s.find('e');
    const int exp10 = atoi(s.c_str() + epos + 1);
    std::string digits;
    for (size_t i = 0; i < epos; ++i)
        if (s[i] != '.') digits.push_back(s[i]);
    const double a = std::fabs(v);
    std::string out;
    if (a >= 1e-3 && a < 1e7) {
        if (exp10 >= 0) {
            std::string ip = digits.substr(0, std::min<size_t>(digits.size(), (size_t)exp10 + 1));
            while ((int)ip.size() < exp10 + 1) ip.push_back('0');
            std::string fp = digits.size() > (size_t)exp10 + 1 ? digits.substr(exp10 + 1) : "0";
            out = ip + "." + fp;
        } else {
            out = "0." + std::string((size_t)(-exp10 - 1), '0') + digits;
        }
    } else {
        out = digits.substr(0, 1) + "." + (digits.size() > 1 ? digits.substr(1) : "0") + "E" + std::to_string(exp10);
    }
    return sign + out;
}

// Creates `path` and writes n_rows pieces of text, one write each: fill_line(i, line) appends piece i to the empty
// `line`.
template <class Fill>
int write_lines(const char* path, int64_t n_rows, Fill fill_line) {
    std::unique_ptr<FILE, int (*)(FILE*)> f(fopen(path, "wb"), fclose);
    if (!f) return fail(ALS_ERR_IO, "cannot create %s", path);
    std::string line;
    for (int64_t i = 0; i < n_rows; ++i) {
        line.clear();
        fill_line(i, line);
        if (fwrite(line.data(), 1, line.size(), f.get()) != line.size()) return fail(ALS_ERR_IO, "write failed: %s", path);
    }
    if (fclose(f.release()) != 0) return fail(ALS_ERR_IO, "close failed: %s", path);
    return ALS_OK;
}

// EJML MatrixIO.saveDenseCSV of the widened matrix; cell(i, j) yields the fp32 prediction.
template <class Cell>
int write_csv(const char* path, int64_t n_users, int64_t n_movies, Cell cell) {
    return write_lines(path, std::max<int64_t>(n_users, 0) + 1, [&](int64_t i, std::string& line) {
        if (i == 0) {   // the header, then row i - 1
            line = std::to_string((long long)n_users) + " " + std::to_string((long long)n_movies) + " real\n";
            return;
        }
        for (int64_t j = 0; j < n_movies; ++j) (line += java_double((double)cell(i - 1, j))) += ' ';
        line += '\n';
    });
}

}  // namespace

extern "C" {

int als_write_prediction_csv(const char* path, const float* U, int64_t n_users, int64_t ldu, const float* M,
                             int64_t n_movies, int64_t ldm, int num_features) {
    if (!path || (n_users > 0 && !U) || (n_movies > 0 && !M) || num_features < 1 || ldu < num_features ||
        ldm < num_features)
        return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    return write_csv(path, n_users, n_movies, [&](int64_t i, int64_t j) {
        const float* x = U + i * ldu;
        const float* y = M + j * ldm;
        float total = 0.f;   // MatrixMatrixMult_FDRM.multTransB: sequential fp32 dot
        for (int c = 0; c < num_features; ++c) total += x[c] * y[c];
        return total;
    });
}

int als_write_prediction_matrix_csv(const char* path, const float* P, int64_t n_users, int64_t n_movies) {
    if (!path || n_users < 0 || n_movies < 0 || (n_users > 0 && n_movies > 0 && !P))
        return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    return write_csv(path, n_users, n_movies, [&](int64_t i, int64_t j) { return P[i * n_movies + j]; });
}

int als_write_recommendations_csv(const char* path, const int64_t* user_ids, int64_t n_users, int top_n,
                                  const int64_t* movie_ids, const float* scores) {
    if (!path || n_users < 0 || top_n < 1 || (n_users > 0 && (!user_ids || !movie_ids || !scores)))
        return fail(ALS_ERR_INVALID_ARGUMENT, "bad arguments");
    return write_lines(path, n_users, [&](int64_t i, std::string& line) {
        for (int j = 0; j < top_n; ++j) {
            const int64_t m = movie_ids[i * top_n + j];
            if (m < 0) continue;
            (line += std::to_string((long long)user_ids[i])) += ',';
            (line += std::to_string((long long)m)) += ',';
            (line += java_double((double)scores[i * top_n + j])) += '\n';
        }
    });
}

}  // extern "C"
