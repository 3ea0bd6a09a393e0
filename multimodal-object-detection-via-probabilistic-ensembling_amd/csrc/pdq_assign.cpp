// pe_pdq_assign (host, float64): the one-to-one assignment of ground truths to detections that maximises the sum of the pair qualities
// of pe_pdq_pair_quality (csrc/pdq.hip), image by image.  DESIGN.md section 30.
//
// The Hungarian algorithm in its O(n^2 m) shortest-augmenting-path form with row and column potentials, on the cost -q: the rows are the
// shorter side of the image's block (ground truths that take part x detections that take part), so either orientation is one code path.
// No device work: the file has no kernel, and the entry point touches no HIP call.
#include <stdint.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "proben_hip.h"

// Not csrc/common.h: it includes the HIP runtime, and this file is also built without it, by a host compiler under
// -fsanitize=address,undefined beside tests/csrc/pdq_assign_check.cpp.  Hence the declaration and the macro below, copies of common.h's.
namespace pe {
void set_error(const char* fmt, ...);
}

#define PE_CHECK_ARG(cond, ...)                  \
    do {                                         \
        if (!(cond)) {                           \
            pe::set_error(__VA_ARGS__);          \
            return PE_ERR_INVALID_ARG;           \
        }                                        \
    } while (0)

namespace {

// cost [n][m] row-major, n <= m: col_of[i] = the column of row i in an assignment of every row that minimises the total cost
void hungarian(const std::vector<double>& cost, int n, int m, std::vector<int>& col_of) {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> u(n + 1, 0.0), v(m + 1, 0.0), minv(m + 1);
    std::vector<int> p(m + 1, 0), way(m + 1, 0);       // p[j] = the row (1-based) that holds column j, 0 = free
    std::vector<char> used(m + 1);
    for (int i = 1; i <= n; ++i) {
        p[0] = i;
        int j0 = 0;
        std::fill(minv.begin(), minv.end(), inf);
        std::fill(used.begin(), used.end(), 0);
        do {
            used[j0] = 1;
            const int i0 = p[j0];
            double delta = inf;
            int j1 = 0;
            for (int j = 1; j <= m; ++j) {
                if (used[j]) continue;
                const double cur = cost[(size_t)(i0 - 1) * m + (j - 1)] - u[i0] - v[j];
                if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
                if (minv[j] < delta) { delta = minv[j]; j1 = j; }
            }
            for (int j = 0; j <= m; ++j) {
                if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
                else minv[j] -= delta;
            }
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const int j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0 != 0);
    }
    col_of.assign(n, -1);
    for (int j = 1; j <= m; ++j)
        if (p[j] > 0) col_of[p[j] - 1] = j - 1;
}

}  // namespace

extern "C" int pe_pdq_assign(const double* q_host, const int32_t* gt_live_host, const int32_t* det_take_host, const int32_t* det_offsets_host,
                             const int32_t* gt_offsets_host, const int64_t* pair_offsets_host, int32_t num_images, int32_t num_dets,
                             int32_t num_gt, int64_t num_pairs, int32_t* out_match_host) {
    PE_CHECK_ARG(num_images >= 0 && num_dets >= 0 && num_gt >= 0 && num_pairs >= 0,
                 "pe_pdq_assign: num_images %d, num_dets %d, num_gt %d, num_pairs %lld: a negative count", num_images, num_dets, num_gt,
                 (long long)num_pairs);
    PE_CHECK_ARG(num_images > 0 || (num_dets == 0 && num_gt == 0 && num_pairs == 0), "pe_pdq_assign: %d detections, %d ground truths and "
                 "%lld pairs without images", num_dets, num_gt, (long long)num_pairs);
    if (num_images == 0) return PE_OK;
    PE_CHECK_ARG(det_offsets_host && gt_offsets_host && pair_offsets_host, "pe_pdq_assign: null pointer (det_offsets / gt_offsets / pair_offsets)");
    PE_CHECK_ARG(num_gt == 0 || (gt_live_host && out_match_host), "pe_pdq_assign: null pointer (gt_live / out_match)");
    PE_CHECK_ARG(num_pairs == 0 || q_host, "pe_pdq_assign: null pointer (q)");
    PE_CHECK_ARG(det_offsets_host[0] == 0 && gt_offsets_host[0] == 0 && pair_offsets_host[0] == 0, "pe_pdq_assign: offsets do not start at 0");
    for (int b = 0; b < num_images; ++b) {
        const int64_t Mb = (int64_t)det_offsets_host[b + 1] - det_offsets_host[b], Gb = (int64_t)gt_offsets_host[b + 1] - gt_offsets_host[b];
        PE_CHECK_ARG(Mb >= 0 && Gb >= 0, "pe_pdq_assign: offsets of image %d are not monotone (detections %d..%d, ground truths %d..%d)", b,
                     det_offsets_host[b], det_offsets_host[b + 1], gt_offsets_host[b], gt_offsets_host[b + 1]);
        PE_CHECK_ARG(pair_offsets_host[b + 1] - pair_offsets_host[b] == Gb * Mb, "pe_pdq_assign: pair_offsets of image %d span %lld pairs for "
                     "%lld ground truths x %lld detections", b, (long long)(pair_offsets_host[b + 1] - pair_offsets_host[b]), (long long)Gb,
                     (long long)Mb);
    }
    PE_CHECK_ARG(det_offsets_host[num_images] == num_dets && gt_offsets_host[num_images] == num_gt && pair_offsets_host[num_images] == num_pairs,
                 "pe_pdq_assign: offsets end at %d / %d / %lld for %d detections, %d ground truths, %lld pairs", det_offsets_host[num_images],
                 gt_offsets_host[num_images], (long long)pair_offsets_host[num_images], num_dets, num_gt, (long long)num_pairs);
    for (int g = 0; g < num_gt; ++g) out_match_host[g] = -1;
    std::vector<int> rows, cols, col_of;
    std::vector<double> cost;
    for (int b = 0; b < num_images; ++b) {
        const int d0 = det_offsets_host[b], Mb = det_offsets_host[b + 1] - d0, g0 = gt_offsets_host[b], Gb = gt_offsets_host[b + 1] - g0;
        const double* q = q_host + pair_offsets_host[b];
        rows.clear();
        cols.clear();
        for (int k = 0; k < Gb; ++k)
            if (gt_live_host[g0 + k] != 0) rows.push_back(k);
        for (int j = 0; j < Mb; ++j)
            if (!det_take_host || det_take_host[d0 + j] != 0) cols.push_back(j);
        const int R = (int)rows.size(), C = (int)cols.size();
        if (R == 0 || C == 0) continue;
        // the shorter side becomes the rows of the cost; a pair quality that is not finite and > 0 is worth nothing
        const bool flip = R > C;
        const int n = flip ? C : R, m = flip ? R : C;
        cost.assign((size_t)n * m, 0.0);
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < C; ++j) {
                const double x = q[(size_t)rows[i] * Mb + cols[j]];
                cost[flip ? (size_t)j * m + i : (size_t)i * m + j] = x > 0.0 && x < std::numeric_limits<double>::infinity() ? -x : 0.0;
            }
        hungarian(cost, n, m, col_of);
        for (int i = 0; i < n; ++i) {
            const int gi = flip ? col_of[i] : i, dj = flip ? i : col_of[i];
            if (cost[(size_t)i * m + col_of[i]] < 0.0) out_match_host[g0 + rows[gi]] = d0 + cols[dj];
        }
    }
    return PE_OK;
}
