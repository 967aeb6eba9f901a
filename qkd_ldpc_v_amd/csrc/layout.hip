// layout.hip — from H to the decoder's index tables, on the host.
//
// Graph planning: the Tanner graph of H (the reference's H_matrix,
// src/array_and_matrix_operations.hpp:60-77) is turned once into the decoder's
// lane partition — E edges in CSR order dealt EPL-per-lane to T lanes — plus a
// row-ELL copy for syndrome checks.  build_layout validates the adjacency,
// chooses the plan (plan.hip) and fills a GraphTables stage by stage; capi.hip
// replicates the tables on each device of the graph.  Nothing here touches a
// device.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "graph.hpp"
#include "relabel.hpp"

namespace qldpc {
namespace {

// Labellings already searched in this process (relabel.cpp takes ~0.5 s on a
// 10k code; tests and drivers create graphs of one H many times).  Keyed by a
// hash of everything the search reads, verified by a full compare on a hit.
struct RelabelMemo {
    std::vector<int32_t> key;  // n, m, waves, mode, iters, row_ptr..., col_idx...
    std::vector<int32_t> lab;
    long long stats[4];
};
std::mutex g_relabel_mu;
std::vector<RelabelMemo> g_relabel_memo;  // most recent last, at most 8

// 64-bit FNV-1a over the plan's scalars (listed here by hand) and every
// `digested` table of QLDPC_GRAPH_TABLES (graph.hpp) in the list's order, each
// table as its element count (uint64) and raw bytes: what tests/test_layout.py
// pins.  A table added to the list is hashed unless its entry says otherwise.
// Known gap: the five frame-per-lane tables are listed but not digested — the
// recorded digests predate them, and even an empty table hashes its count, so
// no value recorded from a parent could include them.  The CPU suite does not
// see their contents.
uint64_t layout_digest(const qldpc_graph &g, const GraphTables &t) {
    uint64_t h = 0xcbf29ce484222325ull;
    auto bytes = [&](const void *p, size_t nb) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < nb; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    };
    auto i32 = [&](int32_t v) { bytes(&v, sizeof v); };
    auto tab = [&](const auto &v) {
        const uint64_t cnt = v.size();
        bytes(&cnt, sizeof cnt);
        if (cnt) bytes(v.data(), v.size() * sizeof(v[0]));
    };
    for (int v : {g.n, g.m, g.E, g.variant, g.T, g.EPL, g.dv_max, g.max_dc, g.v2R, g.v2RG, g.n_iso, g.vn_k0, g.n_hd,
                  g.hd_uniform_dv, g.nst_max, g.split_k, g.split_mrows, g.split_cb, g.split_nc, g.split_pl,
                  g.rows_lds_ms, g.rows_lds_waves_ms})
        i32(v);
    for (bool b : {g.vng, g.paired, g.rows_global_ms}) i32(b ? 1 : 0);
    const int64_t sd = g.stage_doubles;
    bytes(&sd, sizeof sd);
#define QLDPC_X(type, name, when, digested) if (digested) tab(t.name);
    QLDPC_GRAPH_TABLES(QLDPC_X)
#undef QLDPC_X
    return h;
}

// One graph's layout under construction: the adjacency, the plan (g) and what
// the stages hand on to each other.  build() runs the stages in order.
struct Layout {
    const int32_t n, m;
    const int32_t *const row_ptr, *const col_idx;
    const int32_t *const col_ptr, *const row_idx;  // bit_nodes in the caller's order, or NULL
    const int E;
    qldpc_graph *const g;
    GraphTables &t;
    const int layout;  // QLDPC_LAYOUT_*

    // classify
    std::vector<int> dv;
    // choose_plan
    int T = 0, EPL = 0;
    // edge_order: the slot geometry and the layout's row-major edge list
    std::vector<int> row_of, kpos;
    bool v2 = false, reg = false;
    int G4 = 0, TS = 0, NPARTS = 0, W = 0;
    uint32_t DUMMY = 0;
    std::vector<int> lrp, lrow, ledge, perm;
    // relabel
    std::vector<int32_t> col_r;
    const int32_t *colL = nullptr;  // the metadata's bit ids
    // vn_stage
    std::vector<int32_t> rank;
    int S4 = 0;  // V2 slots per lane (register + scratch)
    // bit_gather
    long long vng_chunks = 0;
    std::vector<long long> P0;
    bool vng_h = false;
    // slot layouts
    int nst_max = 0;

    size_t midx(int l, int k) const {
        return ((size_t)((l / TS) * G4 + k / 4) * TS + (size_t)(l % TS)) * 4 + (size_t)(k % 4);
    }

    // Validate the adjacency and classify it: degrees, sorted rows, bit_nodes
    // the ascending transpose or not (occurrence pairing).
    int classify() {
        dv.assign(n, 0);
        bool rows_sorted = true;
        for (int j = 0; j < m; ++j) {
            g->max_dc = std::max(g->max_dc, row_ptr[j + 1] - row_ptr[j]);
            for (int e = row_ptr[j]; e < row_ptr[j + 1]; ++e) {
                const int c = col_idx[e];
                if (c < 0 || c >= n) return fail(QLDPC_EINVAL, "col_idx entry out of range [0, n)");
                if (e > row_ptr[j] && col_idx[e - 1] >= c) rows_sorted = false;
                ++dv[c];
            }
        }
        // The reference pairs a check's k-th input with the k-th time the VN loop
        // visits that check (bit_pos_idx, src/qkd_ldpc_algorithm.cpp:116-118) and
        // a bit's k-th message with the k-th check that reached it (check_pos_idx,
        // :67-69).  With ascending check_nodes rows and bit_nodes their ascending
        // transpose both pairings are the edge itself; otherwise an edge's b2c is
        // total - c2b of the edge the counters pair it with (occurrence pairing).
        if (!rows_sorted) {
            for (int j = 0; j < m; ++j) {  // (a bit listed twice in one check is not supported)
                std::vector<int32_t> r(col_idx + row_ptr[j], col_idx + row_ptr[j + 1]);
                std::sort(r.begin(), r.end());
                if (std::adjacent_find(r.begin(), r.end()) != r.end())
                    return fail(QLDPC_EUNSUP, "a check node lists the same bit twice");
            }
        }
        bool cols_transpose = true;
        if (col_ptr && row_idx) {
            if (col_ptr[0] != 0 || col_ptr[n] != row_ptr[m])
                return fail(QLDPC_EUNSUP, "bit_nodes and check_nodes hold different edge counts");
            std::vector<int> cnt(m, 0);
            for (int i = 0; i < n; ++i) {
                if (col_ptr[i + 1] < col_ptr[i]) return fail(QLDPC_EINVAL, "col_ptr must be non-decreasing");
                if (col_ptr[i + 1] - col_ptr[i] != dv[i])
                    return fail(QLDPC_EUNSUP, "bit_nodes and check_nodes disagree on a bit's degree");
                for (int e = col_ptr[i]; e < col_ptr[i + 1]; ++e) {
                    const int j = row_idx[e];
                    if (j < 0 || j >= m) return fail(QLDPC_EINVAL, "row_idx entry out of range [0, m)");
                    ++cnt[j];
                }
            }
            for (int j = 0; j < m; ++j)
                if (cnt[j] != row_ptr[j + 1] - row_ptr[j])
                    return fail(QLDPC_EUNSUP, "bit_nodes and check_nodes disagree on a check's degree");
            // bit_nodes[c] must list the checks holding c in ascending order (the
            // order the check-node loop reaches c in) for the identity pairing
            std::vector<int> fill(n, 0);
            for (int j = 0; j < m && cols_transpose; ++j)
                for (int e = row_ptr[j]; e < row_ptr[j + 1]; ++e) {
                    const int c = col_idx[e];
                    if (row_idx[col_ptr[c] + fill[c]++] != j) {
                        cols_transpose = false;
                        break;
                    }
                }
        }
        g->paired = !(rows_sorted && cols_transpose);
        for (int i = 0; i < n; ++i) g->dv_max = std::max(g->dv_max, dv[i]);
        {
            long long chunks = 0;
            for (int i = 0; i < n; ++i) chunks += (dv[i] + 3) / 4;
            g->vng_h_fit = chunks + V2_VNG_DUMMY_CHUNKS <= V2_CODES_CAP && g->dv_max < 256;
        }
        if (g->dv_max >= MAX_DV) return fail(QLDPC_EUNSUP, "a bit node has degree >= 511");
        return QLDPC_OK;
    }

    int choose_plan() {
        // QLDPC_VARIANT=v1 keeps the first-generation planner (comparison / tests).
        const char *want = qldpc_diag_env("QLDPC_VARIANT");
        const bool v1_only = want && std::strcmp(want, "v1") == 0;
        if (g->paired && want && std::strcmp(want, "v2") == 0)
            return fail(QLDPC_EUNSUP, "QLDPC_VARIANT=v2 but the adjacency needs occurrence pairing (v1)");
        if (v1_only || g->paired || (!plan_v2(*g, row_ptr) && !plan_v2_split(*g, row_ptr, col_idx))) plan(*g);
        if (want && std::strcmp(want, "v2") == 0 && g->variant != VAR_V2)
            return fail(QLDPC_EUNSUP, "QLDPC_VARIANT=v2 but no V2 instantiation holds this graph");
        T = g->T;
        EPL = g->EPL;
        for (int i = 0; i < n; ++i)
            if (dv[i] == 0) t.iso_bits.push_back(i);
        g->n_iso = (int)t.iso_bits.size();
        return QLDPC_OK;
    }

    void edge_order() {
        // Lane partition metadata.
        std::vector<int> seen(n, 0);
        row_of.resize(E);
        kpos.resize(E);
        for (int j = 0; j < m; ++j)
            for (int e = row_ptr[j]; e < row_ptr[j + 1]; ++e) {
                row_of[e] = j;
                kpos[e] = seen[col_idx[e]]++;
            }
        // uint4 groups per lane, group-major [g][lane][4]; the register variants
        // have a fixed group count at lane stride REG_TSTRIDE.
        v2 = g->variant == VAR_V2;
        reg = g->variant == VAR_REG_LDS || v2;
        G4 = v2 ? (g->v2R + g->v2RG) / 4 : (reg ? EPL_REG / 4 : (EPL + 3) / 4);
        TS = reg ? REG_TSTRIDE : T;
        NPARTS = (T + TS - 1) / TS;  // V2 split: parts of TS lanes, each its own [G4][TS][4] block
        S4 = G4 * 4;
        t.slot_meta.assign((size_t)G4 * TS * 4 * NPARTS, 0);
        t.lane_row0.assign(T, v2 ? 0 : -1);
        t.lane_head.assign(T, 0);
        t.lane_nst.assign(T, 0);
        t.lane_epl.assign(T, EPL);
        // Lane l holds edges [e_begin, e_end) of its wave (v1: one "wave" of T lanes).
        // V2 metadata differs in three ways: the END of a lane's tail (a row begun
        // in the lane before) is cleared — the kernel finishes split rows after a
        // shuffle; slots past the lane's edges up to the group count are dummy
        // edges (column n, kpos META_KPOS_MASK, no flags), so every lane of a wave
        // runs the same slots; lanes count the rows they start (lane_nst).
        DUMMY = (uint32_t)n | (META_KPOS_MASK << META_KPOS_SHIFT);
        W = v2 ? T / 64 : 1;
        // V2 min-sum metadata lists each row's edges by kpos: the min-sum row
        // aggregate and parity are order-free, and grouping a
        // row's k-th bit edges lets the VN phase masks skip more slots.  SPA keeps
        // CSR order (its row product is sequential, :57-62).
        // Layout order: V2 relabels rows (plan_v2 balances waves); lrp / lrow /
        // ledge give, per position of the layout's row-major edge list, its row
        // and its original CSR edge.  v1 keeps the original order.
        lrp.assign(row_ptr, row_ptr + m + 1);
        lrow = row_of;
        ledge.resize(E);
        perm.resize(E);
        for (int e = 0; e < E; ++e) ledge[e] = e;
        if (v2) {
            lrp = g->layout_row_ptr;
            for (int j = 0; j < m; ++j) {
                const int r = g->row_order[j];
                for (int t = 0; t < row_ptr[r + 1] - row_ptr[r]; ++t) {
                    lrow[lrp[j] + t] = j;
                    ledge[lrp[j] + t] = row_ptr[r] + t;
                }
            }
            t.row_orig.assign(g->row_order.begin(), g->row_order.end());
        }
    }

    // Bank-aware relabelling of bit ids (relabel.cpp), one-workgroup register
    // shapes: the (wave, slot, half) groups of both slot layouts (CSR order for
    // the SPA family, kpos order for min-sum) read total[label] with distinct
    // banks, and the min-sum bit gather's code-word ORs (dv <= 4) hit distinct
    // banks too.  The metadata, vn_rows and vng_rec then carry labels; the frame
    // codes are written in label order and the decoder maps its outputs back.
    // QLDPC_RELABEL=0: identity (A/B).
    void relabel() {
        colL = col_idx;
        const int relabel_mode = env_int("QLDPC_RELABEL", 1);  // (A/B: 2 CSR layout only, 3 kpos layout only)
        if (v2 && g->split_k <= 1 && g->v2RG == 0 && relabel_mode != 0) {
            const bool word = v2_vng_ok(2, g->v2R, g->v2RG, g->split_k, g->dv_max, m);
            std::vector<RelabelGroup> groups;
            for (int sorted = 0; sorted < 2; ++sorted) {
                if ((relabel_mode == 2 && sorted) || (relabel_mode == 3 && !sorted)) continue;
                std::vector<int> pm(ledge);
                if (sorted)
                    for (int j = 0; j < m; ++j)
                        std::stable_sort(pm.begin() + lrp[j], pm.begin() + lrp[j + 1],
                                         [&](int x, int y) { return kpos[x] < kpos[y]; });
                for (int w = 0; w < T / 64; ++w) {
                    const long long wb = lrp[g->wave_rows[w]], we = lrp[g->wave_rows[w + 1]];
                    const int epl_w = std::max<int>((int)((we - wb + 63) / 64), g->max_dc);
                    if (we == wb) continue;
                    for (int k = 0; k < epl_w; ++k)
                        for (int h = 0; h < 2; ++h) {
                            RelabelGroup grp;
                            for (int li = 32 * h; li < 32 * h + 32; ++li) {
                                const long long e = wb + (long long)li * epl_w + k;
                                if (e < we) {
                                    const int ed = pm[e];
                                    grp.members.push_back({col_idx[ed], 0, (uint8_t)(1 | ((sorted && word && kpos[ed] < 4) ? 2 : 0))});
                                } else {
                                    grp.members.push_back({-1, n % 128, 1});  // dummy slot: column n
                                }
                            }
                            groups.push_back(std::move(grp));
                        }
                }
            }
            const int iters = env_int("QLDPC_RELABEL_ITERS", 16);  // search moves per edge
            std::vector<int32_t> key = {n, m, T / 64, relabel_mode, iters};
            key.insert(key.end(), row_ptr, row_ptr + m + 1);
            key.insert(key.end(), col_idx, col_idx + E);
            {
                std::lock_guard<std::mutex> lk(g_relabel_mu);
                for (const auto &me : g_relabel_memo)
                    if (me.key == key) {
                        g->col_lab = me.lab;
                        std::copy(me.stats, me.stats + 4, g->relabel_stats);
                        break;
                    }
            }
            if (g->col_lab.empty()) {
                RelabelStats st;
                g->col_lab = bank_relabel(n, groups, 0x5eed0ba4c5ull, (long long)iters * E, &st);
                g->relabel_stats[0] = st.excess_before;
                g->relabel_stats[1] = st.excess_after;
                g->relabel_stats[2] = st.cycles_before;
                g->relabel_stats[3] = st.cycles_after;
                std::lock_guard<std::mutex> lk(g_relabel_mu);
                if (g_relabel_memo.size() >= 8) g_relabel_memo.erase(g_relabel_memo.begin());
                g_relabel_memo.push_back({std::move(key), g->col_lab, {g->relabel_stats[0], g->relabel_stats[1],
                                                                        g->relabel_stats[2], g->relabel_stats[3]}});
            }
            col_r.resize(E);
            for (int e = 0; e < E; ++e) col_r[e] = g->col_lab[col_idx[e]];
            colL = col_r.data();
        }
    }

    // Hybrid shape: VN terms kk >= vn_k0 go through a per-frame stage, laid out
    // term-major over the bits of degree > kk, bits ordered by degree
    // (descending) so each term's bits are a prefix: stage[off[kk] + rank[b]].
    void vn_stage() {
        auto &hd_bits = t.hd_bits, &hd_dv = t.hd_dv, &stage_off = t.stage_off;
        g->vn_k0 = g->dv_max;
        stage_off.assign(std::max(1, g->dv_max), 0);
        rank.assign(n, -1);
        // (split frames: every term goes through the stage, and the gather pass
        // adds them to the channel LLR in order: the message pass stores only)
        if (v2 && ((g->v2RG > 0 && g->dv_max > 4) || (g->split_k > 1 && g->dv_max >= 1))) {
            g->vn_k0 = g->split_k > 1 ? 0 : 4;
            for (int i = 0; i < n; ++i)
                if (dv[i] > g->vn_k0) hd_bits.push_back(i);
            std::stable_sort(hd_bits.begin(), hd_bits.end(), [&](int x, int y) { return dv[x] > dv[y]; });
            for (size_t i = 0; i < hd_bits.size(); ++i) {
                rank[hd_bits[i]] = (int)i;
                hd_dv.push_back(dv[hd_bits[i]]);
            }
            long long off = 0;
            for (int kk = g->vn_k0; kk < g->dv_max; ++kk) {
                stage_off[kk] = (int32_t)off;
                for (int d : hd_dv) off += (d > kk) ? 1 : 0;
            }
            g->stage_doubles = off;
        }
        g->n_hd = (int)hd_bits.size();
        if (g->n_hd == n && n > 0) {
            bool uni = true;
            for (int i = 0; i < n && uni; ++i) uni = hd_bits[i] == i && hd_dv[i] == hd_dv[0];
            g->hd_uniform_dv = (uni && env_int("QLDPC_HD_TABLES", 0) == 0) ? hd_dv[0] : 0;  // (env: A/B)
        }
    }

    // Min-sum bit gather (VNG).  Register shape, dv <= 4: per bit, the layout
    // rows of its kpos-th edge (u16 each, 0xFFFF past its degree).  Hybrid
    // shape: a bit's edges padded to chunks of four (position P0[b] + kpos),
    // rows per chunk (padding: row 0), each slot's position (vng_meta2; dummy
    // slots: a scratch chunk per lane past the last), bits in degree order.
    void bit_gather() {
        auto &vn_rows = t.vn_rows, &vng_bits = t.vng_bits, &vng_meta2 = t.vng_meta2, &vng_rec = t.vng_rec;
        P0.assign(v2 ? n : 0, 0);
        if (v2 && v2_vng_ok(2, g->v2R, g->v2RG, g->split_k, g->dv_max, m)) {
            std::vector<int> lrow_of(m, 0);
            for (int j = 0; j < m; ++j) lrow_of[g->row_order[j]] = j;
            if (g->v2RG == 0) {
                vn_rows.assign((size_t)2 * n, 0xFFFFFFFFu);
                for (int r = 0; r < m; ++r)
                    for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
                        uint32_t &w = vn_rows[(size_t)2 * colL[e] + (kpos[e] >> 1)];
                        const int sh = 16 * (kpos[e] & 1);
                        w = (w & ~(0xFFFFu << sh)) | ((uint32_t)lrow_of[r] << sh);
                    }
            } else {
                for (int b = 0; b < n; ++b) {
                    P0[b] = vng_chunks * 4;
                    vng_chunks += (dv[b] + 3) / 4;
                }
                if (vng_chunks + V2_VNG_DUMMY_CHUNKS <= V2_CODES_CAP && g->dv_max < 256) {
                    vn_rows.assign((size_t)2 * vng_chunks, 0u);
                    for (int r = 0; r < m; ++r)
                        for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
                            const long long P = P0[col_idx[e]] + kpos[e];
                            vn_rows[(size_t)(P >> 1)] |= (uint32_t)lrow_of[r] << (16 * (P & 1));
                        }
                    std::vector<int> ord(n);
                    for (int b = 0; b < n; ++b) ord[b] = b;
                    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return dv[x] > dv[y]; });
                    // Thread t gathers positions t, t + T, ...: wave w's lanes take
                    // the 64-bit groups at j T + 64 w.  Groups of 64 consecutive
                    // bits in degree order (similar chunk counts: no lane idles
                    // long) are dealt longest-first to the wave with the least
                    // work so far, so the gather's barrier does not wait on the
                    // waves that drew the high-degree bits (QLDPC_VNG_DEAL=0: in
                    // order).  Only full rounds are dealt; the rest stays in order.
                    const int TW = g->T / 64, rounds = n / g->T;
                    if (env_int("QLDPC_VNG_DEAL", 1) && TW > 1 && rounds > 1) {
                        const int ng = rounds * TW;
                        std::vector<long long> load(TW, 0);
                        std::vector<int> used(TW, 0), dst(ng);
                        for (int gi = 0; gi < ng; ++gi) {  // groups come longest first
                            const long long cost = (dv[ord[(size_t)gi * 64]] + 3) / 4;
                            int best = -1;
                            for (int w = 0; w < TW; ++w)
                                if (used[w] < rounds && (best < 0 || load[w] < load[best])) best = w;
                            dst[gi] = used[best]++ * g->T + 64 * best;
                            load[best] += cost;
                        }
                        std::vector<int> dealt(ord);
                        for (int gi = 0; gi < ng; ++gi)
                            for (int l = 0; l < 64; ++l) dealt[dst[gi] + l] = ord[(size_t)gi * 64 + l];
                        ord.swap(dealt);
                    }
                    vng_bits.resize((size_t)2 * n);
                    for (int i = 0; i < n; ++i) {
                        vng_bits[2 * i] = (uint32_t)ord[i];
                        vng_bits[2 * i + 1] = (uint32_t)(P0[ord[i]] / 4) | ((uint32_t)dv[ord[i]] << 24);
                    }
                    vng_meta2.assign((size_t)G4 * TS * 4 * NPARTS, 0);
                }
            }
        }
        vng_h = !vng_meta2.empty();
        // Register-shape bit gather: per slot where the message pass ORs the
        // edge's two bits — the byte offset of the bit's code word and the
        // shift of its kpos-th bit pair (8 (col & 3) + 2 kpos).
        if (v2 && !vn_rows.empty() && g->v2RG == 0) vng_rec.assign((size_t)G4 * TS * 4 * NPARTS, 0);
        g->vng = !vn_rows.empty();
    }

    // One slot layout (CSR order, or each row's edges sorted by kpos) and its VN
    // masks.  Scan row structure (V2; row boundaries are the same in the CSR and
    // the kpos-sorted layout): per wave and slot the lanes whose slot starts /
    // ends a row, and (min-sum) parks its tail aggregate (lane masks the scan
    // tests as scalar registers),
    // and per lane the slot mask of each row it starts (bit 63: the row
    // continues into the next lane) for the row parities of the decisions.
    int build_meta(bool sorted, std::vector<uint32_t> &mt, std::vector<uint64_t> &vnm, std::vector<uint32_t> &mt2,
                   std::vector<uint64_t> &vex) {
        auto &lrow0 = t.lane_row0, &lhead = t.lane_head, &lnst = t.lane_nst, &lepl = t.lane_epl;
        auto &stage_off = t.stage_off;
        auto &vng_meta2 = t.vng_meta2, &vng_rec = t.vng_rec;
        auto &row_sem = t.row_sem, &row_rmask = t.row_rmask;
        const bool rowstruct = v2 && !sorted && g->split_k <= 1 && g->v2RG == 0 && S4 <= 63;
        std::vector<std::vector<uint64_t>> rm(rowstruct ? T : 0);
        if (rowstruct) row_sem.assign((size_t)W * S4 * 4, 0);
        mt.assign((size_t)G4 * TS * 4 * NPARTS, 0);
        // (the hybrid shape's SPA message pass loads a slot_meta2 word beside every
        // slot_meta word, staged terms or not: with dv_max <= 4 there is no stage
        // and the words stay 0, but the table must span the slots)
        mt2.assign((g->n_hd || (v2 && g->v2RG > 0)) ? (size_t)G4 * TS * 4 * NPARTS : 0, 0);
        vnm.assign(v2 ? (size_t)W * g->dv_max : 0, 0);
        vex.assign(v2 ? (size_t)W * g->dv_max * S4 : 0, 0);
        perm = ledge;
        if (sorted)
            for (int j = 0; j < m; ++j)
                std::stable_sort(perm.begin() + lrp[j], perm.begin() + lrp[j + 1],
                                 [&](int x, int y) { return kpos[x] < kpos[y]; });
        for (int w = 0; w < W; ++w) {
            const long long wb = v2 ? lrp[g->wave_rows[w]] : 0;
            const long long we = v2 ? lrp[g->wave_rows[w + 1]] : E;
            const int lanes = v2 ? 64 : T;
            const int epl_w = v2 ? std::max<int>((int)((we - wb + 63) / 64), g->max_dc) : EPL;
            for (int li = 0; li < lanes; ++li) {
                const int l = w * 64 + li;
                const long long e0 = wb + (long long)li * epl_w;
                if (v2) lepl[l] = epl_w;
                int head = 0;
                lnst[l] = 0;
                if (e0 < we) {
                    const int r0 = lrow[e0];
                    lrow0[l] = r0;
                    if (e0 != lrp[r0]) head = lhead[l] = lrp[r0 + 1] - (int)e0;
                }
                for (int k = 0; k < (v2 ? G4 * 4 : epl_w); ++k) {
                    const long long e = e0 + k;  // position in the row-major edge list
                    uint32_t wd;
                    if (k >= epl_w || e >= we) {
                        if (!v2) break;
                        wd = DUMMY;
                        if (sorted && vng_h) vng_meta2[midx(l, k)] = (uint32_t)((vng_chunks + li) * 4);
                        // register-shape bit gather: dummy slots record into the
                        // spare word past the per-bit bytes (V2Layout::syn)
                        if (sorted && !vng_rec.empty()) vng_rec[midx(l, k)] = (uint32_t)((n + 3) & ~3);
                    } else {
                        const int j = lrow[e];
                        const int ed = perm[e];  // the edge at that position
                        wd = (uint32_t)colL[ed] | ((uint32_t)kpos[ed] << META_KPOS_SHIFT) | META_VALID;
                        if (v2) {
                            vnm[(size_t)w * g->dv_max + kpos[ed]] |= 1ull << k;
                            vex[((size_t)w * g->dv_max + kpos[ed]) * S4 + k] |= 1ull << li;
                        }
                        if (sorted && vng_h) vng_meta2[midx(l, k)] = (uint32_t)(P0[col_idx[ed]] + kpos[ed]);
                        if (sorted && !vng_rec.empty() && kpos[ed] < 4) {
                            const uint32_t c = (uint32_t)colL[ed];
                            vng_rec[midx(l, k)] = (c & ~3u) | ((((c & 3u) << 3) + 2u * (uint32_t)kpos[ed]) << 16);
                        }
                        if (g->n_hd && kpos[ed] >= g->vn_k0)
                            mt2[midx(l, k)] =
                                (uint32_t)(stage_off[kpos[ed]] + rank[col_idx[ed]]);
                        if (e == lrp[j]) {
                            wd |= META_START;
                            ++lnst[l];
                            if (rowstruct) {
                                row_sem[((size_t)w * S4 + k) * 4] |= 1ull << li;
                                // slots of this row in the lane; bit 63 when it runs past the lane
                                const long long last = std::min<long long>(lrp[j + 1] - 1, e0 + epl_w - 1);
                                uint64_t msk = 0;
                                for (long long q = e; q <= last; ++q) msk |= 1ull << (q - e0);
                                if (lrp[j + 1] - 1 > e0 + epl_w - 1) msk |= 1ull << 63;
                                rm[l].push_back(msk);
                            }
                        }
                        if (e == lrp[j + 1] - 1 && !(v2 && k < head)) {
                            wd |= META_END;
                            if (rowstruct) row_sem[((size_t)w * S4 + k) * 4 + 1] |= 1ull << li;
                        }
                    }
                    mt[midx(l, k)] = wd;
                    // min-sum: a lane's tail aggregate (a row begun in the lane
                    // before) is parked at slot `head` — its first START, or a
                    // dummy slot when the wave's edges end with the tail
                    if (rowstruct && head > 0 && k == head && k < S4)
                        row_sem[((size_t)w * S4 + k) * 4 + 2] |= 1ull << li;
                }
            }
        }
        if (rowstruct) {
            for (auto &v : rm) nst_max = std::max(nst_max, (int)v.size());
            row_rmask.assign((size_t)std::max(nst_max, 1) * T, 0);
            for (int l = 0; l < T; ++l)
                for (size_t j = 0; j < rm[l].size(); ++j) row_rmask[j * T + l] = rm[l][j];
        }
        return QLDPC_OK;
    }

    // Occurrence pairing (unsorted adjacency, v1 global-slot layout: edge e at
    // lane e / EPL, slot e % EPL, message index slot * T + lane).  The VN loop
    // (:109-120) visits bit i's checks in bit_nodes order; its jj-th visit of
    // check r fills r's next input slot with total[i] - c2b[i][jj], and
    // c2b[i][jj] is the message of the jj-th check (in check order) holding i
    // (:67-69).  pair_src / pair_col: per input slot, that message's index and i.
    int pairing() {
        auto &pair_src = t.pair_src, &pair_col = t.pair_col;
        if (g->paired) {
            if (v2) return fail(QLDPC_EUNSUP, "occurrence pairing needs the v1 layout");
            auto aidx = [&](int e) { return (e % EPL) * T + e / EPL; };
            std::vector<int> cbase(n + 1, 0);
            for (int i = 0; i < n; ++i) cbase[i + 1] = cbase[i] + dv[i];
            std::vector<int> edge_of(E);  // (bit, occurrence rank) -> edge
            for (int e = 0; e < E; ++e) edge_of[cbase[col_idx[e]] + kpos[e]] = e;
            std::vector<int32_t> cp(cbase.begin(), cbase.end()), ri(E);
            if (col_ptr && row_idx) {
                cp.assign(col_ptr, col_ptr + n + 1);
                ri.assign(row_idx, row_idx + E);
            } else {  // bit_nodes = the ascending transpose
                std::vector<int> fill(n, 0);
                for (int j = 0; j < m; ++j)
                    for (int e = row_ptr[j]; e < row_ptr[j + 1]; ++e) ri[cbase[col_idx[e]] + fill[col_idx[e]]++] = j;
            }
            pair_src.assign((size_t)EPL * T, 0);
            pair_col.assign((size_t)EPL * T, 0);
            std::vector<int> bpos(m, 0);
            for (int i = 0; i < n; ++i)
                for (int jj = 0; jj < dv[i]; ++jj) {
                    const int r = ri[cp[i] + jj];
                    const int e_dst = row_ptr[r] + bpos[r]++;
                    pair_src[aidx(e_dst)] = aidx(edge_of[cbase[i] + jj]);
                    pair_col[aidx(e_dst)] = i;
                }
        }
        return QLDPC_OK;
    }

    // The two slot layouts: CSR order (SPA family) and, V2, kpos order (min-sum).
    int slot_layouts() {
        int brc = build_meta(false, t.slot_meta, t.vn_mask, t.slot_meta2, t.vn_exec);
        if (!brc && v2) brc = build_meta(true, t.slot_meta_ms, t.vn_mask_ms, t.slot_meta2_ms, t.vn_exec_ms);
        if (brc) return brc;
        g->nst_max = t.row_sem.empty() ? 0 : nst_max;
        return QLDPC_OK;
    }

    // Split frames' exchange layout (DecodeArgs::xoff): each staged term's
    // region is (owner part of its bit, chunk, kpos); inside a region the terms
    // follow (writer wave, slot, lane), so the stage position of every slot is
    // assigned walking the slots in that order.  Region sizes depend only on
    // the edges, so both slot layouts (CSR, kpos-sorted) share xoff.
    int split_exchange() {
        auto &xoff = t.xoff;
        if (v2 && g->split_k > 1 && g->split_cb > 0) {
            const int K = g->split_k, NC = g->split_nc, CB = g->split_cb, D = g->dv_max;
            std::vector<int32_t> reg0(n), lbit(n);
            for (int p = 0; p < K; ++p) {
                const int lo = (int)((long long)n * p / K), hi = (int)((long long)n * (p + 1) / K);
                for (int b = lo; b < hi; ++b) {
                    const int c = (b - lo) / CB;
                    reg0[b] = (p * NC + c) * D;
                    lbit[b] = (b - lo) - c * CB;
                }
            }
            const size_t NR = (size_t)K * NC * D;
            std::vector<long long> fill(NR + 1, 0);
            for (int e = 0; e < E; ++e) ++fill[(size_t)reg0[col_idx[e]] + kpos[e] + 1];
            for (size_t r = 0; r < NR; ++r) fill[r + 1] += fill[r];
            if (fill[NR] != g->stage_doubles) return fail(QLDPC_EUNSUP, "split exchange layout: term count");
            xoff.assign(fill.begin(), fill.end());
            fill.pop_back();
            // Order inside a region: (writer part, slot group of four, wave, slot,
            // lane) — the 16 waves of a part, which run the message pass roughly
            // in step, fill one run per region and slot group together, so a
            // region has one or two open L2 lines per part instead of one per
            // wave.  QLDPC_SPLIT_XORDER=0: (wave, slot, lane), one run per wave (A/B).
            const bool grouped = env_int("QLDPC_SPLIT_XORDER", 1) != 0;
            const int WPp = REG_TSTRIDE / 64;  // waves per part
            auto assign = [&](const std::vector<uint32_t> &mt, std::vector<uint32_t> &mt2, std::vector<uint16_t> &xb) {
                std::vector<long long> pos(fill);
                xb.assign((size_t)g->stage_doubles, 0);
                auto place = [&](int w, int k) {
                    for (int li = 0; li < 64; ++li) {
                        const size_t i = midx(w * 64 + li, k);
                        const uint32_t kp = (mt[i] >> META_KPOS_SHIFT) & META_KPOS_MASK;
                        if (kp == META_KPOS_MASK) continue;  // dummy slot
                        const int b = (int)(mt[i] & META_COL_MASK);
                        const long long q = pos[(size_t)reg0[b] + kp]++;
                        mt2[i] = (uint32_t)q;
                        xb[(size_t)q] = (uint16_t)lbit[b];
                    }
                };
                if (grouped) {
                    for (int p = 0; p < K; ++p)
                        for (int k0 = 0; k0 < S4; k0 += 4)
                            for (int w = p * WPp; w < std::min(W, (p + 1) * WPp); ++w)
                                for (int k = k0; k < k0 + 4; ++k) place(w, k);
                } else {
                    for (int w = 0; w < W; ++w)
                        for (int k = 0; k < S4; ++k) place(w, k);
                }
            };
            assign(t.slot_meta, t.slot_meta2, t.xbit);
            assign(t.slot_meta_ms, t.slot_meta2_ms, t.xbit_ms);
        }
        return QLDPC_OK;
    }

    void print_plan() const {  // host-side plan statistics on stderr
        auto visited = [&](const std::vector<uint64_t> &v) {
            long long s = 0;
            for (int w = 0; w < W; ++w)
                for (int kk = 1; kk < g->dv_max; ++kk) s += __builtin_popcountll(v[(size_t)w * g->dv_max + kk]);
            return s;
        };
        long long full = 0;
        for (int w = 0; w < W; ++w) full += (long long)(g->dv_max - 1) * t.lane_epl[w * 64];
        fprintf(stderr, "{\"plan\": {\"waves\": %d, \"slots_reg\": %d, \"slots_scratch\": %d, \"epl_max\": %d, "
                        "\"dv_max\": %d, \"vn_slot_visits_csr\": %lld, \"vn_slot_visits_kpos_sorted\": %lld, "
                        "\"vn_slot_visits_unmasked\": %lld, \"rows_global_ms\": %d, \"rows_lds_ms\": %d, "
                        "\"rows_lds_waves_ms\": %d, \"split_k\": %d, \"split_cb\": %d, \"split_nc\": %d}}\n",
                W, g->v2R, g->v2RG, g->EPL, g->dv_max, visited(t.vn_mask), visited(t.vn_mask_ms), full,
                (int)g->rows_global_ms, g->rows_lds_ms, g->rows_lds_waves_ms, g->split_k, g->split_cb, g->split_nc);
        fprintf(stderr, "{\"relabel\": {\"excess_before\": %lld, \"excess_after\": %lld, \"cycles_before\": %lld, "
                        "\"cycles_after\": %lld}}\n",
                g->relabel_stats[0], g->relabel_stats[1], g->relabel_stats[2], g->relabel_stats[3]);
    }

    // Row-ELL (slot-major) for syndrome evaluation, and (relabelled graphs) its
    // copy in labels with the inverse labelling.
    void row_ell() {
        auto &ell = t.ell_col, &rdeg = t.row_deg, &ell_lab = t.ell_lab, &col_orig = t.col_orig;
        const int dcm = std::max(1, g->max_dc);
        ell.assign((size_t)dcm * std::max(m, 1), 0);
        rdeg.assign(std::max(m, 1), 0);
        for (int j = 0; j < m; ++j) {
            rdeg[j] = row_ptr[j + 1] - row_ptr[j];
            for (int k = 0; k < rdeg[j]; ++k) ell[(size_t)k * m + j] = col_idx[row_ptr[j] + k];
        }

        if (!g->col_lab.empty()) {
            ell_lab = ell;
            for (int j = 0; j < m; ++j)
                for (int k = 0; k < rdeg[j]; ++k) ell_lab[(size_t)k * m + j] = g->col_lab[ell[(size_t)k * m + j]];
            col_orig.resize(n);
            for (int i = 0; i < n; ++i) col_orig[g->col_lab[i]] = i;
        }
    }

    // Frame-per-lane (decoder_fpl.hip): the adjacency itself is the layout —
    // CSR rows, each edge's position in bit_nodes order (the identity pairing:
    // a bit's k-th message comes from the k-th row holding it) and the CSC
    // starts.  Labels stay the reference's bit ids.
    int build_fpl() {
        if (g->paired)
            return fail(QLDPC_EUNSUP, "the frame-per-lane layout needs ascending check_nodes rows and bit_nodes their "
                                      "ascending transpose; this adjacency needs the reference's occurrence pairing "
                                      "(v1 kernels, QLDPC_LAYOUT_AUTO)");
        g->variant = VAR_FPL;
        g->T = FPL_LANES;
        g->EPL = 0;
        for (int i = 0; i < n; ++i)
            if (dv[i] == 0) t.iso_bits.push_back(i);
        g->n_iso = (int)t.iso_bits.size();
        t.fpl_row_ptr.assign(row_ptr, row_ptr + m + 1);
        t.fpl_col.assign(col_idx, col_idx + E);
        t.fpl_col_ptr.assign(n + 1, 0);
        for (int i = 0; i < n; ++i) t.fpl_col_ptr[i + 1] = t.fpl_col_ptr[i] + dv[i];
        t.fpl_cslot.resize(E);
        std::vector<int> seen(n, 0);
        for (int e = 0; e < E; ++e) t.fpl_cslot[e] = t.fpl_col_ptr[col_idx[e]] + seen[col_idx[e]]++;
        // rows by length class, in row order inside a class (decoder.hpp FPL_CLASS_CAP)
        for (int c = 0; c <= FPL_CLASSES; ++c) g->fpl_class_off[c] = 0;
        for (int j = 0; j < m; ++j) ++g->fpl_class_off[fpl_row_class(row_ptr[j + 1] - row_ptr[j]) + 1];
        for (int c = 0; c < FPL_CLASSES; ++c) g->fpl_class_off[c + 1] += g->fpl_class_off[c];
        t.fpl_rows.resize(m);
        {
            std::vector<int> fill(g->fpl_class_off, g->fpl_class_off + FPL_CLASSES);
            for (int j = 0; j < m; ++j) t.fpl_rows[fill[fpl_row_class(row_ptr[j + 1] - row_ptr[j])]++] = j;
        }
        row_ell();  // (the frame builders and the deal's weights read the row-ELL)
        return QLDPC_OK;
    }

    int build() {
        int rc;
        if ((rc = classify())) return rc;
        if (layout == QLDPC_LAYOUT_FRAME_PER_LANE) return build_fpl();
        if ((rc = choose_plan())) return rc;
        edge_order();
        relabel();
        vn_stage();
        bit_gather();
        if ((rc = pairing()) || (rc = slot_layouts()) || (rc = split_exchange())) return rc;
        const bool debug = qldpc_diag_env("QLDPC_DEBUG_PLAN") != nullptr;
        if (v2 && debug) print_plan();
        row_ell();
        // the planner's own tables, as the devices get them
        t.part_row0.assign(g->part_row0.begin(), g->part_row0.end());
        t.wave_rows.assign(g->wave_rows.begin(), g->wave_rows.end());
        t.col_lab = g->col_lab;
        if (debug)
            fprintf(stderr, "{\"layout\": {\"digest\": \"%016llx\"}}\n", (unsigned long long)layout_digest(*g, t));
        return QLDPC_OK;
    }
};

}  // namespace

// bit_nodes (col_ptr / row_idx, the reference's H_matrix::bit_nodes in its
// own order): NULL means the ascending transpose of check_nodes.
int build_layout(int32_t n, int32_t m, const int32_t *row_ptr, const int32_t *col_idx, const int32_t *col_ptr,
                 const int32_t *row_idx, std::unique_ptr<qldpc_graph> &out, GraphTables &t, int layout) {
    if (n <= 0 || m < 0 || !row_ptr || (!col_idx && row_ptr[m] > 0))
        return fail(QLDPC_EINVAL, "invalid graph dimensions or NULL arrays");
    if (n > MAX_N) return fail(QLDPC_EUNSUP, "n exceeds 2^20 bit nodes");
    if (row_ptr[0] != 0) return fail(QLDPC_EINVAL, "row_ptr[0] must be 0");
    for (int j = 0; j < m; ++j)
        if (row_ptr[j + 1] < row_ptr[j]) return fail(QLDPC_EINVAL, "row_ptr must be non-decreasing");
    const int E = row_ptr[m];
    if (E <= 0) return fail(QLDPC_EINVAL, "graph has no edges");
    // QLDPC_VARIANT=fpl (diagnostic switch) selects the frame-per-lane layout as the option does
    if (const char *want = qldpc_diag_env("QLDPC_VARIANT"))
        if (std::strcmp(want, "fpl") == 0) layout = QLDPC_LAYOUT_FRAME_PER_LANE;
    // Empty check rows: before the first and after the last non-empty row only
    // (v1 decodes those; a lane's row counter steps by one per row start, so
    // an empty row between two others is refused wherever it falls).  The
    // frame-per-lane layout walks rows by row_ptr and takes them anywhere.
    if (layout != QLDPC_LAYOUT_FRAME_PER_LANE) {
        int first = 0, last = m - 1;
        while (row_ptr[first + 1] == row_ptr[first]) ++first;
        while (row_ptr[last + 1] == row_ptr[last]) --last;
        for (int j = first; j <= last; ++j)
            if (row_ptr[j + 1] == row_ptr[j])
                return fail(QLDPC_EUNSUP, "empty check rows between non-empty rows are not supported");
    }

    auto g = std::make_unique<qldpc_graph>();
    g->n = n;
    g->m = m;
    g->E = E;
    Layout L{n, m, row_ptr, col_idx, col_ptr, row_idx, E, g.get(), t, layout};
    if (int rc = L.build()) return rc;
    if (qldpc_diag_env("QLDPC_DEBUG_PLAN")) print_launch_shapes(*g);  // (every variant, after its plan / layout lines)
    out = std::move(g);
    return QLDPC_OK;
}

}  // namespace qldpc
