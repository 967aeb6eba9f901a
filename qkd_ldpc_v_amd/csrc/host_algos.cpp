// host_algos.cpp — the C ABI entries that are host arithmetic only (no GPU, no
// HIP header): the reference's generator and seeds, rate adaptation, untainted
// puncturing and the simulation driver's helpers, each consuming the generator
// exactly as the reference does.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../include/qkd_ldpc_hip.h"

namespace qldpc {
int fail(int code, const std::string &msg);  // capi.hip (declared in graph.hpp, which needs the HIP headers)
}
using qldpc::fail;

namespace {
// Xoshiro256++ (Blackman & Vigna) with Xoshiro-cpp v1.1's seeding (four
// SplitMix64 outputs) — a UniformRandomBitGenerator, so std::shuffle /
// std::uniform_int_distribution consume it exactly as the reference does.
struct Xoshiro256pp {
    using result_type = uint64_t;
    uint64_t s[4];
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    explicit Xoshiro256pp(uint64_t seed) {
        uint64_t x = seed;
        for (auto &v : s) {
            uint64_t z = (x += 0x9e3779b97f4a7c15ull);
            z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
            z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
            v = z ^ (z >> 31);
        }
    }
    static constexpr result_type min() { return 0; }
    static constexpr result_type max() { return ~(uint64_t)0; }
    result_type operator()() {
        const uint64_t r = rotl(s[0] + s[3], 23) + s[0];
        const uint64_t t = s[1] << 17;
        s[2] ^= s[0];
        s[3] ^= s[1];
        s[1] ^= s[2];
        s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl(s[3], 45);
        return r;
    }
};
}  // namespace

extern "C" {

double qldpc_log_p(double qber) { return std::log((1. - qber) / qber); }

// ---- rate adaptation (src/array_and_matrix_operations.cpp:1131-1223) ----------
int qldpc_xoshiro_state(uint64_t seed, uint64_t *state_out) {
    if (!state_out) return fail(QLDPC_EINVAL, "NULL state_out");
    Xoshiro256pp g(seed);
    for (int i = 0; i < 4; ++i) state_out[i] = g.s[i];
    return QLDPC_OK;
}

int qldpc_adapt_code_rate(int32_t n, int32_t m, double qber, double delta, double efficiency,
                          int32_t untainted_enabled, const int32_t *untainted, int32_t n_untainted,
                          uint64_t *prng_state, int32_t *punctured_out, int32_t *n_punctured, int32_t *shortened_out,
                          int32_t *n_shortened, double *adapted_rate_out) {
    if (n <= 0 || m < 0 || m >= n || !prng_state || !n_punctured || !n_shortened)
        return fail(QLDPC_EINVAL, "bad dimensions or NULL outputs");
    if (untainted_enabled && n_untainted > 0 && !untainted) return fail(QLDPC_EINVAL, "NULL untainted list");
    *n_punctured = 0;
    *n_shortened = 0;
    if (adapted_rate_out) *adapted_rate_out = 0.;
    Xoshiro256pp g(0);
    for (int i = 0; i < 4; ++i) g.s[i] = prng_state[i];
    const double h_b = -qber * std::log2(qber) - (1. - qber) * std::log2(1. - qber);
    const double optimal_R = 1. - efficiency * h_b;
    const double original_R = 1. - static_cast<double>(m) / static_cast<double>(n);
    const int num_short = static_cast<int>(std::ceil((original_R - optimal_R * (1. - delta)) * static_cast<double>(n)));
    const int num_punct = static_cast<int>(delta * static_cast<double>(n) - static_cast<double>(num_short));
    // beyond the achievable range: the reference warns and skips the combination
    if (num_short <= 0 || num_punct <= 0) return QLDPC_OK;
    std::vector<int> punct, bit_positions(n);
    if (untainted_enabled) {
        if (num_punct > n_untainted) return QLDPC_OK;
        punct.assign(untainted, untainted + num_punct);
    } else {
        for (int i = 0; i < n; ++i) bit_positions[i] = i;
        std::shuffle(bit_positions.begin(), bit_positions.end(), g);
        punct.assign(bit_positions.begin(), bit_positions.begin() + num_punct);
    }
    std::sort(punct.begin(), punct.end());
    for (int i = 0; i < n; ++i) bit_positions[i] = i;
    std::vector<int> remaining(n - num_punct);
    std::set_difference(bit_positions.begin(), bit_positions.end(), punct.begin(), punct.end(), remaining.begin());
    std::shuffle(remaining.begin(), remaining.end(), g);
    std::vector<int> shortened(remaining.begin(), remaining.begin() + num_short);
    std::sort(shortened.begin(), shortened.end());
    for (int i = 0; i < 4; ++i) prng_state[i] = g.s[i];
    *n_punctured = num_punct;
    *n_shortened = num_short;
    if (punctured_out) std::copy(punct.begin(), punct.end(), punctured_out);
    if (shortened_out) std::copy(shortened.begin(), shortened.end(), shortened_out);
    if (adapted_rate_out)
        *adapted_rate_out = static_cast<double>(n - m - num_short) / static_cast<double>(n - num_punct - num_short);
    return QLDPC_OK;
}

// ---- untainted puncturing (src/array_and_matrix_operations.cpp:975-1067) -----
// select_punctured_bits_untainted (arXiv:1103.6149): while untainted bits
// remain (X), take the bits of X with the fewest second-order neighbours
// (bits sharing a check, the bit itself excluded: get_second_order_neighbors,
// :975-996) inside X, in ascending order (std::set iteration), draw one with
// uniform_int_distribution<size_t>(0, candidates - 1) from the caller's
// generator, puncture it and remove it and its second-order neighbours from
// X.  Same candidates, same draws, same order as the reference's set-scanning
// loop; the counts |N2(i) n X| are kept incrementally instead of recounted
// (the relation is symmetric, so removing r decrements every q in N2(r)).
int qldpc_select_punctured_untainted(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx,
                                     const int32_t *col_ptr, const int32_t *row_idx, uint64_t *prng_state,
                                     int32_t *punctured_out, int32_t *n_punctured) {
    if (n <= 0 || m < 0 || !row_ptr || !col_idx || !col_ptr || !row_idx || !prng_state || !n_punctured)
        return fail(QLDPC_EINVAL, "bad dimensions or NULL arguments");
    *n_punctured = 0;
    if (row_ptr[m] != col_ptr[n]) return fail(QLDPC_EINVAL, "check_nodes / bit_nodes edge counts differ");
    for (int j = 0; j < m; ++j)
        for (int e = row_ptr[j]; e < row_ptr[j + 1]; ++e)
            if (col_idx[e] < 0 || col_idx[e] >= n) return fail(QLDPC_EINVAL, "bit index out of range");
    for (int i = 0; i < n; ++i)
        for (int e = col_ptr[i]; e < col_ptr[i + 1]; ++e)
            if (row_idx[e] < 0 || row_idx[e] >= m) return fail(QLDPC_EINVAL, "check index out of range");
    // N2(i): sorted, unique, without i
    std::vector<int64_t> n2p(n + 1, 0);
    std::vector<int32_t> n2;
    {
        std::vector<int32_t> tmp;
        for (int i = 0; i < n; ++i) {
            tmp.clear();
            for (int e = col_ptr[i]; e < col_ptr[i + 1]; ++e) {
                const int j = row_idx[e];
                tmp.insert(tmp.end(), col_idx + row_ptr[j], col_idx + row_ptr[j + 1]);
            }
            std::sort(tmp.begin(), tmp.end());
            tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
            for (int32_t b : tmp)
                if (b != i) n2.push_back(b);
            n2p[i + 1] = (int64_t)n2.size();
        }
    }
    Xoshiro256pp g(0);
    for (int i = 0; i < 4; ++i) g.s[i] = prng_state[i];
    std::vector<uint8_t> inx(n, 1);
    std::vector<int32_t> cnt(n), xs(n), cand, punct;
    for (int i = 0; i < n; ++i) cnt[i] = (int32_t)(n2p[i + 1] - n2p[i]);
    for (int i = 0; i < n; ++i) xs[i] = i;  // X in ascending order (compacted lazily)
    auto remove = [&](int r) {
        if (!inx[r]) return;
        inx[r] = 0;
        for (int64_t q = n2p[r]; q < n2p[r + 1]; ++q) --cnt[n2[q]];
    };
    while (!xs.empty()) {
        size_t w = 0;
        int32_t min_n = n;  // (the reference starts its minimum at num_bit_nodes)
        for (int32_t i : xs)
            if (inx[i]) {
                xs[w++] = i;
                if (cnt[i] < min_n) min_n = cnt[i];
            }
        xs.resize(w);
        if (xs.empty()) break;
        cand.clear();
        for (int32_t i : xs)
            if (cnt[i] == min_n) cand.push_back(i);
        std::uniform_int_distribution<size_t> d(0, cand.size() - 1);
        const int chosen = cand[d(g)];
        punct.push_back(chosen);
        remove(chosen);
        for (int64_t q = n2p[chosen]; q < n2p[chosen + 1]; ++q) remove(n2[q]);
    }
    for (int i = 0; i < 4; ++i) prng_state[i] = g.s[i];
    *n_punctured = (int32_t)punct.size();
    if (punctured_out) std::copy(punct.begin(), punct.end(), punctured_out);
    return QLDPC_OK;
}

// ---- simulation-driver helpers (src/config.cpp, src/array_and_matrix_operations.cpp:121-256) ----
int qldpc_sort_permutation(const double *keys, int32_t n, int32_t *perm_out) {
    if (n < 0 || (n > 0 && (!keys || !perm_out))) return fail(QLDPC_EINVAL, "bad n / NULL arrays");
    // The reference sorts config structs by code_rate with std::sort (not
    // stable): the same libstdc++ algorithm on the same key sequence moves the
    // elements identically, so the permutation of (key, index) pairs is theirs.
    std::vector<std::pair<double, int32_t>> v(n);
    for (int32_t i = 0; i < n; ++i) v[i] = {keys[i], i};
    std::sort(v.begin(), v.end(), [](const std::pair<double, int32_t> &a, const std::pair<double, int32_t> &b) {
        return a.first < b.first;
    });
    for (int32_t i = 0; i < n; ++i) perm_out[i] = v[i].second;
    return QLDPC_OK;
}

int qldpc_bits_to_remove(int32_t n, int32_t m, const int32_t *col_ptr, const int32_t *row_idx, int32_t n_punct,
                         const int32_t *punctured, int32_t n_short, const int32_t *shortened, int32_t rate_adapt,
                         int32_t *out, int32_t *count) {
    if (n <= 0 || m < 0 || !col_ptr || !row_idx || !count || (n_punct && !punctured) || (n_short && !shortened))
        return fail(QLDPC_EINVAL, "bad arguments");
    // find_available_index over a marked-check bitmap (same first-unmarked choice
    // as std::find over the marked list, in O(E) overall).
    std::vector<char> marked(m, 0);
    auto take = [&](int i) -> bool {
        for (int e = col_ptr[i]; e < col_ptr[i + 1]; ++e)
            if (!marked[row_idx[e]]) {
                marked[row_idx[e]] = 1;
                return true;
            }
        return false;
    };
    std::vector<int> removed;
    std::vector<std::pair<int, int>> cand;  // (bit, column weight)
    if (rate_adapt) {  // get_bits_positions_to_remove_rate_adapt (:189-256)
        int s = 0, p = 0;
        for (int i = 0; i < n; ++i) {
            if (s < n_short && shortened[s] == i) {
                removed.push_back(i);
                ++s;
            } else if (p < n_punct && punctured[p] == i) {
                removed.push_back(i);
                take(i);
                ++p;
            } else {
                cand.push_back({i, col_ptr[i + 1] - col_ptr[i]});
            }
        }
    } else {  // get_bits_positions_to_remove (:138-185)
        for (int i = 0; i < n; ++i) cand.push_back({i, col_ptr[i + 1] - col_ptr[i]});
    }
    // std::sort by column weight (not stable): same algorithm, same order as the reference
    std::sort(cand.begin(), cand.end(),
              [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.second < b.second; });
    for (const auto &c : cand)
        if (take(c.first)) removed.push_back(c.first);
    std::sort(removed.begin(), removed.end());
    *count = (int32_t)removed.size();
    if (out) std::copy(removed.begin(), removed.end(), out);
    return QLDPC_OK;
}

// ---- trial generator (src/simulation.cpp:540-551,713-719,743) ----------------
int qldpc_trial_seeds(uint64_t simulation_seed, int32_t count, uint64_t *seeds_out) {
    if (count < 0 || (count > 0 && !seeds_out)) return fail(QLDPC_EINVAL, "bad count / NULL seeds_out");
    // The reference draws seeds with uniform_int_distribution<size_t>(0,
    // SIZE_MAX), which passes each 64-bit output through unchanged.
    Xoshiro256pp g(simulation_seed);
    std::uniform_int_distribution<size_t> d(0, std::numeric_limits<size_t>::max());
    for (int32_t i = 0; i < count; ++i) seeds_out[i] = d(g);
    return QLDPC_OK;
}


// ---- the batch seam of the simulation loop (src/simulation.cpp:721-746) ------
int qldpc_shard_range(int32_t count, int32_t shards, int32_t shard, int32_t *lo, int32_t *hi) {
    if (count < 0 || shards <= 0 || shard < 0 || shard >= shards || !lo || !hi)
        return fail(QLDPC_EINVAL, "bad count / shards / shard / NULL bounds");
    // contiguous slices of ceil(count / shards); trailing shards may be short or empty
    const int64_t per = ((int64_t)count + shards - 1) / shards;
    *lo = (int32_t)std::min<int64_t>(count, (int64_t)shard * per);
    *hi = (int32_t)std::min<int64_t>(count, (int64_t)*lo + per);
    return QLDPC_OK;
}

}  // extern "C"
