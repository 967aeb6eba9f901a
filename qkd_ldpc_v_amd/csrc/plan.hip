// plan.hip — the planners: which kernel variant decodes a graph, with how many
// lanes and slots per lane, and (V2) how its rows are dealt to waves and parts.
// Host arithmetic only; layout.hip builds the tables of the plan chosen here.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "graph.hpp"

// The planner's and the launches' A/B knobs (QLDPC_SPLIT_K, QLDPC_VNG, ...)
// are read only under the diagnostic switch QLDPC_DIAG=1: without it the
// product ignores every QLDPC_* tuning variable, so a stray variable in a
// user's environment cannot change the plan the reference's driver gets.
const char *qldpc::qldpc_diag_env(const char *name) {
    const char *d = std::getenv("QLDPC_DIAG");
    if (!d || std::strcmp(d, "1") != 0) return nullptr;
    return std::getenv(name);
}

namespace qldpc {

int env_int(const char *name, int dflt) {
    const char *v = qldpc_diag_env(name);
    return (v && *v) ? std::atoi(v) : dflt;
}

static int round_up64(long long x) { return (int)(((x + 63) / 64) * 64); }

// Choose (variant, T, EPL).  EPL >= max_dc keeps any row within two lanes;
// lanes past the last edge simply hold no slots.
void plan(qldpc_graph &g) {
    const long long E = g.E;
    const int dcm = std::max(1, g.max_dc);
    // Register-resident messages: at most EPL_REG edges per lane.  (Occurrence
    // pairing reads other lanes' messages: global-slot variants only.)
    if (dcm <= EPL_REG && !g.paired) {
        const int T = std::max(64, round_up64((E + EPL_REG - 1) / EPL_REG));
        const int EPL = std::max((int)((E + T - 1) / T), dcm);
        if (T <= 1024 && EPL <= EPL_REG && lds_bytes_for(VAR_REG_LDS, g.n, g.m, T) <= LDS_LIMIT) {
            g.variant = VAR_REG_LDS;
            g.T = T;
            g.EPL = EPL;
            return;
        }
    }
    // Messages in global scratch: as many lanes as the workgroup allows.
    const int T = (int)std::min<long long>(1024, std::max(64, round_up64((E + 7) / 8)));
    g.T = T;
    g.EPL = std::max((int)((E + T - 1) / T), dcm);
    g.variant = (lds_bytes_for(VAR_GLB_LDS, g.n, g.m, T) <= LDS_LIMIT) ? VAR_GLB_LDS : VAR_GLB_GLB;
}

namespace {

// Deal rows to W waves so that every wave's edge count is at most cap when
// possible: contiguous blocks of rows first (consecutive check ids keep the
// VN phase masks sparse), then swap / move single rows between the heaviest
// and lightest waves.  Returns wave membership lists and the sums.
// With weights wt, wave w's share of the edges is wt[w] / sum(wt) and its cap
// cap * wt[w] (sums compared as sums[w] / wt[w]).
std::vector<std::vector<int>> balance_rows(const int32_t *row_ptr, int m, int W, long long cap,
                                           std::vector<long long> &sums, const std::vector<double> *wt = nullptr) {
    auto deg = [&](int j) { return row_ptr[j + 1] - row_ptr[j]; };
    const long long E = row_ptr[m];
    std::vector<double> cw(W + 1, 0.0);  // cumulative weights
    for (int w = 0; w < W; ++w) cw[w + 1] = cw[w] + (wt ? (*wt)[w] : 1.0);
    auto wof = [&](int w) { return wt ? (*wt)[w] : 1.0; };
    std::vector<std::vector<int>> waves(W);
    sums.assign(W, 0);
    {
        int j = 0;
        for (int w = 0; w < W; ++w) {
            const long long target = wt ? (long long)std::llround((double)E * cw[w + 1] / cw[W]) : E * (w + 1) / W;
            while (j < m && (w == W - 1 || row_ptr[j + 1] <= target ||
                             (row_ptr[j] < target && target - row_ptr[j] > row_ptr[j + 1] - target))) {
                waves[w].push_back(j);
                sums[w] += deg(j);
                ++j;
            }
        }
    }
    // degree -> rows, per wave
    std::vector<std::map<int, std::vector<int>>> by(W);
    for (int w = 0; w < W; ++w)
        for (int j : waves[w]) by[w][deg(j)].push_back(j);
    for (int iter = 0; iter < 100000; ++iter) {
        int H = 0, L = 0;
        for (int w = 1; w < W; ++w) {
            if (sums[w] / wof(w) > sums[H] / wof(H)) H = w;
            if (sums[w] / wof(w) < sums[L] / wof(L)) L = w;
        }
        if (sums[H] <= (long long)(cap * wof(H)) || H == L) break;
        // (weighted: L's normalised load must stay below H's old one)
        const long long gap = wt ? (long long)((double)sums[H] * wof(L) / wof(H)) - sums[L] : sums[H] - sums[L];
        // best transfer d (row of degree dx from H, optionally one of degree dy from L)
        long long best = 0;
        int bx = -1, by_ = -1;
        for (auto &kx : by[H]) {
            if (kx.second.empty()) continue;
            const long long dx = kx.first;
            if (dx < gap && dx > best) best = dx, bx = kx.first, by_ = -1;  // move
            for (auto &ky : by[L]) {
                if (ky.second.empty()) continue;
                const long long d = dx - ky.first;
                if (d > 0 && d < gap && d > best) best = d, bx = kx.first, by_ = ky.first;
            }
        }
        if (best == 0) break;
        // never overshoot: the new max of the pair must drop
        const int x = by[H][bx].back();
        by[H][bx].pop_back();
        by[L][bx].push_back(x);
        sums[H] -= bx;
        sums[L] += bx;
        if (by_ >= 0) {
            const int y = by[L][by_].back();
            by[L][by_].pop_back();
            by[H][by_].push_back(y);
            sums[L] -= by_;
            sums[H] += by_;
        }
    }
    for (int w = 0; w < W; ++w) {
        waves[w].clear();
        for (auto &kv : by[w]) waves[w].insert(waves[w].end(), kv.second.begin(), kv.second.end());
        std::sort(waves[w].begin(), waves[w].end());
    }
    return waves;
}

// Lane fit of a row deal: wave w holds layout rows [rb[w], rb[w + 1]) (nrp:
// their row_ptr) and deals its edges e = max(ceil(edges / 64), max_dc) per
// lane.  Returns the largest e over the waves, or -1 when a lane would need
// more than R slots or start more than 32 rows (the 32-bit syndrome mask).
int lane_fit(const std::vector<int> &rb, const std::vector<int> &nrp, int W, int max_dc, int R) {
    int epl = 0;
    for (int w = 0; w < W; ++w) {
        const long long ew = nrp[rb[w + 1]] - nrp[rb[w]];
        if (ew == 0) continue;
        const int e = std::max<int>((int)((ew + 63) / 64), max_dc);
        if (e > R) return -1;
        epl = std::max(epl, e);
        for (long long l = 0; l < 64; ++l) {
            const long long e0 = nrp[rb[w]] + l * e, e1 = std::min<long long>(e0 + e, nrp[rb[w + 1]]);
            int starts = 0;
            for (int jr = rb[w]; jr < rb[w + 1]; ++jr)
                if (nrp[jr] >= e0 && nrp[jr] < e1) ++starts;
            if (starts > 32) return -1;
        }
    }
    return epl;
}

}  // namespace

// V2 plan: rows dealt to W waves (balanced by edge count, rows relabelled so
// each wave holds a contiguous block of layout rows), each wave's edges dealt
// EPL_w per lane to its 64 lanes (EPL_w >= max_dc keeps a row within two
// adjacent lanes of ONE wave).  W is the fewest waves whose lanes do not need
// more than max_dc slots (more would only add idle waves and barrier cost),
// capped by the instantiation's workgroup size; the shape is the smallest
// slot count that holds the plan.  QLDPC_V2_WAVES forces W.  Returns false when
// no V2 instantiation fits (v1 is used).
bool plan_v2(qldpc_graph &g, const int32_t *row_ptr) {
    // head <= 31 (tail parity in a 32-bit mask), dummy column id n < 2^20
    if (g.max_dc <= 0 || g.max_dc > 32 || g.n + 1 > (int)META_COL_MASK || g.n > V2_CODES_CAP) return false;
    for (int j = 0; j < g.m; ++j)
        if (row_ptr[j + 1] == row_ptr[j]) return false;  // empty rows: v1 checks them by row-ELL
    const long long E = g.E;
    const int forced = env_int("QLDPC_V2_WAVES", 0);
    const int shapes[4][2] = {{V2_R_TIGHT, 0}, {V2_R_SMALL, 0}, {V2_R_MID, 0}, {V2_R_SMALL, V2_RG_HYBRID}};
    // register shapes (RG == 0) scan from 64-bit lane-mask rows of at most 63
    // slots (row_rmask bit 63 marks a row continuing into the next lane)
    static_assert(V2_R_TIGHT <= 63 && V2_R_SMALL <= 63 && V2_R_MID <= 63, "register shape beyond the scan's masks");
    for (const auto &sh : shapes) {
        const int R = sh[0] + sh[1];  // slots per lane
        const int wmax = v2_threads_for(sh[0]) / 64;
        int W = forced > 0 ? forced : (int)std::min<long long>(wmax, (E + 64LL * g.max_dc - 1) / (64LL * g.max_dc));
        W = std::max(1, W);
        if (W > wmax) continue;
        // min-sum row aggregates (16 B/row) must fit beside the totals; on the
        // hybrid shape they may live in global scratch instead when the bit
        // gather applies (then only the SPA image, 8 B/row, must fit)
        bool rows_global = false;
        // (the shape's own layout: the mask-driven scan's syndrome words exist
        // on the register shapes only)
        const auto lds = [&](int alg, int rows_lds = -1) {
            V2ShapeQuery q;
            q.alg = alg, q.n = g.n, q.rows = g.m, q.threads = W * 64, q.R = sh[0], q.RG = sh[1], q.rows_lds = rows_lds;
            return v2_launch_shape(q).lds_bytes;
        };
        if (lds(2) > LDS_LIMIT) {
            if (sh[1] == 0 || !g.vng_h_fit || g.m >= 0xFFFF || lds(0) > LDS_LIMIT || lds(2, 0) > LDS_LIMIT) continue;
            rows_global = true;
        }
        const long long cap = 64LL * std::max<long long>((E + 64LL * W - 1) / (64LL * W), g.max_dc);
        std::vector<long long> sums;
        std::vector<int> order, rb(W + 1, 0), nrp(g.m + 1, 0);
        int wl = W, epl = 0;
        // Deal the rows with the waves past the first wl given `share` of a
        // wave's edges; false when some lane would exceed the shape.
        auto deal = [&](double share) -> bool {
            std::vector<double> wt(W, 1.0);
            wl = W;
            for (int pass = 0; pass < 6; ++pass) {
                const bool weighted = share != 1.0 && pass > 0;
                const long long capw = weighted ? 64LL * std::max<long long>(
                    (long long)std::ceil((double)E / (wl + (W - wl) * share) / 64.0), g.max_dc) : cap;
                const auto waves = balance_rows(row_ptr, g.m, W, capw, sums, weighted ? &wt : nullptr);
                order.clear();
                for (int w = 0; w < W; ++w) {
                    order.insert(order.end(), waves[w].begin(), waves[w].end());
                    rb[w + 1] = (int)order.size();
                }
                for (int jr = 0; jr < g.m; ++jr)
                    nrp[jr + 1] = nrp[jr] + (row_ptr[order[jr] + 1] - row_ptr[order[jr]]);
                if (!rows_global) break;
                int wn = env_int("QLDPC_ROWS_LDS", 1) ? W : 0;
                while (wn > 0 && lds(2, rb[wn]) > LDS_LIMIT) --wn;
                const bool agree = share == 1.0 || (pass > 0 && wn == wl);
                wl = wn;
                if (agree) break;
                for (int w = 0; w < W; ++w) wt[w] = w < wl ? 1.0 : share;
            }
            epl = lane_fit(rb, nrp, W, g.max_dc, R);
            return epl >= 0;
        };
        // Rows partly in global scratch: the waves whose rows stay in LDS are
        // the leading wl (as many as fit); the others write their rows to L2
        // in the scan and read them back (the gather, and the copy their
        // message pass reads).  Those get a smaller share of a wave's edges
        // so the phase barriers do not wait on them (R=0.5 code: 80% is 4%
        // faster than an even deal and 5% faster than 65%, tools/env_ab.sh)
        // — the smallest share from QLDPC_RGLB_SHARE (percent) up whose deal
        // fits the shape.  wl depends on the deal, so each deal is redone
        // until they agree.
        bool ok = false;
        const int share0 = rows_global ? std::min(100, std::max(10, env_int("QLDPC_RGLB_SHARE", 80))) : 100;
        for (int sp = share0; sp <= 100 && !ok; sp += 5) ok = deal(sp / 100.0);
        if (!ok) continue;
        g.variant = VAR_V2;
        g.v2R = sh[0];
        g.v2RG = sh[1];
        g.rows_global_ms = rows_global;
        g.rows_lds_ms = g.m;
        g.rows_lds_waves_ms = W;
        if (rows_global) {
            // the rows of the leading wl waves stay in LDS beside the totals
            // (QLDPC_ROWS_LDS=0: none, A/B)
            g.rows_lds_waves_ms = wl;
            g.rows_lds_ms = rb[wl];
        }
        g.T = W * 64;
        g.EPL = epl;
        g.wave_rows = rb;
        g.row_order = order;
        g.layout_row_ptr = nrp;
        return true;
    }
    return false;
}

// V2 split plan, for codes whose frame does not fit one CU (totals beyond LDS
// or more edges than 16 waves x 64 lanes x 40 slots): K parts of WR waves
// each (one workgroup per part), rows dealt to the WR K waves as in plan_v2
// (contiguous balanced blocks).  Totals go to global memory.  Parts are 16
// waves (one per CU), or 8 waves (two per CU, half the LDS each) when that
// lets more frames run at once on an XCD's 32 CUs: a frame's time per
// iteration is set by latency, not by its part count (C4 (ii), n = 102400,
// dv = 4: K = 11, 12 and 16 parts of 16 waves decode in the same 24.0-24.1 ms,
// two frames per XCD each — 32 = 2 x 11 + 10 leaves 10 CUs waiting; with
// 8-wave parts K = 21 runs three per XCD).  The graph's per-part arrays keep
// a stride of 16 waves / REG_TSTRIDE lanes either way (8-wave parts leave
// waves 8..15 of each part empty), so part r = waves [16r, 16r + 16).
// QLDPC_SPLIT=0 disables it (v1 is used); QLDPC_SPLIT_K / QLDPC_SPLIT_WP force
// the part count / size.
bool plan_v2_split(qldpc_graph &g, const int32_t *row_ptr, const int32_t *col_idx) {
    if (env_int("QLDPC_SPLIT", 1) == 0) return false;
    if (g.max_dc <= 0 || g.max_dc > 32 || g.n + 1 > (int)META_COL_MASK) return false;
    for (int j = 0; j < g.m; ++j)
        if (row_ptr[j + 1] == row_ptr[j]) return false;
    const long long E = g.E;
    const int WP = REG_TSTRIDE / 64;  // waves per part in the graph's arrays
    // One attempt: K parts of WR waves, V2_R_SPLIT slots per lane in VGPRs /
    // LDS plus RG in per-workgroup global scratch.
    auto attempt = [&](int K, int RG, int WR) -> bool {
        const int R = V2_R_SPLIT + RG;
        const int PL = WR * 64;                                  // the part's lanes (threads)
        const size_t LIM = (size_t)LDS_LIMIT * WR / WP;           // its LDS: 1 or 2 parts per CU
        const int W = WP * K, Wr = WR * K;
        const long long cap = 64LL * std::max<long long>((E + 64LL * Wr - 1) / (64LL * Wr), g.max_dc);
        if (cap > 64LL * R) return false;
        std::vector<long long> sums;
        const auto waves = balance_rows(row_ptr, g.m, Wr, cap, sums);
        std::vector<int> order, rb(W + 1, 0), nrp(g.m + 1, 0);
        for (int w = 0; w < W; ++w) {  // wave w = part w / WP, its (w % WP)-th wave (empty past WR)
            if (w % WP < WR) {
                const auto &wr = waves[(w / WP) * WR + w % WP];
                order.insert(order.end(), wr.begin(), wr.end());
            }
            rb[w + 1] = (int)order.size();
        }
        if ((int)order.size() != g.m) return false;
        for (int j = 0; j < g.m; ++j) nrp[j + 1] = nrp[j] + (row_ptr[order[j] + 1] - row_ptr[order[j]]);
        const int epl = lane_fit(rb, nrp, W, g.max_dc, R);
        if (epl < 0) return false;
        std::vector<int> prow(K + 1);
        int mrows = 0;
        for (int r = 0; r <= K; ++r) prow[r] = rb[std::min(W, r * WP)];
        for (int r = 0; r < K; ++r) mrows = std::max(mrows, prow[r + 1] - prow[r]);
        const auto part = [&](int alg, int gcb) {  // a part's shape at gcb exchange-gather bits
            V2ShapeQuery q;
            q.alg = alg, q.n = g.n, q.rows = mrows, q.threads = PL, q.split_k = K, q.R = V2_R_SPLIT, q.RG = RG, q.gcb = gcb;
            return v2_launch_shape(q);
        };
        if (part(2, 0).lds_bytes > LIM || part(0, 0).lds_bytes > LIM) return false;
        // Exchange gather (DecodeArgs::xoff): the largest LDS chunk of a part's
        // bits every algorithm's layout holds (SPA keeps its LDS message slots
        // when they fit without it), split evenly; QLDPC_SPLIT_X=0: the
        // term-major stage (A/B).
        int cb = 0, nc = 0;
        if (env_int("QLDPC_SPLIT_X", 1)) {
            const int own = (g.n + K - 1) / K;
            const bool rl0 = part(0, 0).RL > 0;
            auto fits = [&](int c) {
                const LaunchShape spa = part(0, c);
                return part(2, c).lds_bytes <= LIM && spa.lds_bytes <= LIM && (!rl0 || spa.RL > 0);
            };
            int lo = 0, hi = std::min(own, 0xFFFF);
            while (lo < hi) {
                const int mid = (lo + hi + 1) / 2;
                if (fits(mid)) lo = mid;
                else hi = mid - 1;
            }
            if (lo >= 256) {
                nc = (own + lo - 1) / lo;
                cb = (own + nc - 1) / nc;
            }
        }
        g.variant = VAR_V2;
        g.v2R = V2_R_SPLIT;
        g.v2RG = RG;
        g.T = W * 64;
        g.EPL = epl;
        g.wave_rows = rb;
        g.row_order = order;
        g.layout_row_ptr = nrp;
        g.split_k = K;
        g.split_mrows = mrows;
        g.part_row0 = prow;
        g.split_cb = cb;
        g.split_nc = nc;
        g.split_pl = PL;
        return true;
    };
    // The smallest feasible K for each part size, then the size that runs more
    // frames per XCD at once (32 CUs: 32 parts of 16 waves or 64 of 8; ties:
    // 8 waves — C4 stand-in, 4 frames per XCD either way: 15 x 8 waves decode
    // as fast as 8 x 16 and the step runs 4% faster, profiles/r05/c4_wp.txt).  (K need not divide an XCD's parts:
    // groups form in claim order and a workgroup joins the next group whenever
    // it finishes a frame.)
    //
    // Scratch message slots (RG = V2_RG_SPLIT, round 6): 52 slots per lane
    // instead of 40 cut the parts per frame by ~1/4, at a cost — each part's
    // passes hold ~1.3x the edges and the scratch slots travel through L2.
    // Four plan families (part size x slot budget), each at its smallest K.
    // Per slot budget the family with the most frames per XCD wins, ties in
    // the measured order (profiles/r06/split_plans/, 2-stream bench, two split
    // launches in flight): without scratch slots 8-wave parts (two per CU),
    // then 16-wave; with them 16-wave parts (one per CU: half the parts per
    // frame), then 8-wave.  The scratch-slot plan is taken when it runs at
    // least 4/3 the frames per XCD of the plan without: C4 (ii) 8w/0 21 parts
    // (3 frames per XCD) 0.59 Gbit/s, 16w/12 8 parts (4) 0.68 <- taken (8w/12
    // 16 parts: 0.62); the stand-in 8w/0 15 parts (4) 0.451 <- kept, 16w/12 6
    // parts (5) 0.457 at 1.4x the HBM+MALL traffic and a slower decode alone
    // (16w/0 8 parts: 0.436, 8w/12 12 parts: 0.437).  QLDPC_SPLIT_WP (8 / 16)
    // and QLDPC_SPLIT_SCRATCH (0 / 1), diagnostic, restrict the families.
    const int kforce = env_int("QLDPC_SPLIT_K", 0);
    const int wforce = env_int("QLDPC_SPLIT_WP", 0);
    const int sforce = env_int("QLDPC_SPLIT_SCRATCH", -1);
    if (wforce && wforce != 16 && wforce != 8) return false;
    auto smallest_k = [&](int WR, int RG) -> int {
        const long long cap_part = (long long)WR * 64 * (V2_R_SPLIT + RG);
        const int kmin = (int)std::max<long long>(2, (E + cap_part - 1) / cap_part);
        if (kforce) return (kforce >= kmin && kforce <= 32 && attempt(kforce, RG, WR)) ? kforce : 0;
        for (int K = kmin; K <= 32; ++K)
            if (attempt(K, RG, WR)) return K;
        return 0;
    };
    struct Plan {
        int K = 0, WR = 0, RG = 0, f = 0;
    };
    auto best_of = [&](int RG, int first_wr) -> Plan {  // the better part size for one slot budget
        Plan b;
        for (int WR : {first_wr, 24 - first_wr}) {
            if (wforce && WR != wforce) continue;
            const int K = smallest_k(WR, RG);
            const int f = K ? (WR == 8 ? 64 : 32) / K : 0;  // frames per XCD (32 CUs)
            if (f > b.f) b = {K, WR, RG, f};                 // (ties keep the first size)
        }
        return b;
    };
    const Plan p0 = sforce == 1 ? Plan{} : best_of(0, 8);
    const Plan ps = sforce == 0 ? Plan{} : best_of(V2_RG_SPLIT, 16);
    const Plan pick = (ps.K && (!p0.K || 3 * ps.f >= 4 * p0.f)) ? ps : p0;
    if (!pick.K) return false;
    return attempt(pick.K, pick.RG, pick.WR);  // (the last attempt sets the plan)
}

// QLDPC_VNG=0 (diagnostic switch, read at every launch): VN phases instead of the min-sum bit gather.
bool vng_enabled() {
    const char *e = qldpc_diag_env("QLDPC_VNG");
    return !(e && std::strcmp(e, "0") == 0);
}

// The launch of (graph, algorithm): a few integer operations, computed per call
// so that a knob flipped between two decodes of one graph is honoured.
LaunchShape launch_shape(const qldpc_graph &g, int alg, bool vng_enabled) {
    if (g.variant == VAR_V2) {
        const bool split = g.split_k > 1;
        V2ShapeQuery q;
        q.alg = alg, q.n = g.n, q.R = g.v2R, q.RG = g.v2RG, q.split_k = g.split_k;
        q.rows = split ? g.split_mrows : g.m;
        q.threads = split ? g.split_pl : g.T;  // one part's lanes, or the graph's
        q.gcb = g.split_cb;
        q.rglb = g.rows_global_ms && alg >= 2;
        if (q.rglb) q.rows_lds = g.rows_lds_ms;
        q.want_vng = g.vng && vng_enabled && v2_vng_ok(alg, g.v2R, g.v2RG, g.split_k, g.dv_max, g.m);
        return v2_launch_shape(q);
    }
    LaunchShape s;
    s.variant = g.variant;
    s.alg = alg;
    s.threads = g.T;  // (frame-per-lane: FPL_LANES; its transposes' LDS is static)
    s.lds_bytes = g.variant == VAR_FPL ? 0 : lds_bytes_for(g.variant, g.n, g.m, g.T);
    return s;
}

const char *LaunchShape::variant_name() const {
    switch (variant) {
    case VAR_REG_LDS: return "reg_lds";
    case VAR_GLB_LDS: return "glb_lds";
    case VAR_V2: return split_k > 1 ? "v2_split" : RG > 0 ? "v2_hybrid" : "v2";
    case VAR_FPL: return "fpl";
    default: return "glb_glb";
    }
}

std::string LaunchShape::name() const {
    char b[128];
    if (variant == VAR_V2)
        snprintf(b, sizeof b, "v2<alg=%d,R=%d,RG=%d,RL=%d,split=%d,pl=%d,vng=%d,rglb=%d>", alg, R, RG, RL, split_k,
                 part_lanes, (int)vng, (int)rglb);
    else snprintf(b, sizeof b, "%s<alg=%d,T=%d>", variant_name(), alg, threads);
    return b;
}

// One {"launch": ...} line per algorithm on stderr (QLDPC_DEBUG_PLAN): what a
// decode of this graph would launch under the knobs as they are now.
void print_launch_shapes(const qldpc_graph &g) {
    for (int alg = 0; alg <= 5; ++alg) {
        const LaunchShape s = launch_shape(g, alg, vng_enabled());
        fprintf(stderr, "{\"launch\": {\"alg\": %d, \"variant\": \"%s\", \"name\": \"%s\", \"threads\": %d, "
                        "\"lanes\": %d, \"lds_bytes\": %zu, \"R\": %d, \"RG\": %d, \"RL\": %d, \"split_k\": %d, "
                        "\"part_lanes\": %d, \"vng\": %d, \"rglb\": %d, \"rows_lds\": %d, \"gcb\": %d}}\n",
                alg, s.variant_name(), s.name().c_str(), s.threads, s.lanes(), s.lds_bytes, s.R, s.RG, s.RL, s.split_k,
                s.part_lanes, (int)s.vng, (int)s.rglb, s.rows_lds, s.gcb);
    }
}

}  // namespace qldpc
