// run_trials.hip — qldpc_run_trials: one combination's trials generated,
// decoded and compared on the graph's devices, each device's slice in chunks
// alternating over two pipeline slots (TrialSlot, graph.hpp).
// ---- the batch seam of the simulation loop (src/simulation.cpp:721-746) ------
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "graph.hpp"

using namespace qldpc;

// One combination's trials in flight: where its results go, and the first
// error of each device's slice.  Its chunks sit in the devices' pipeline slots
// (TrialSlot::owner) until harvested — by qldpc_run_trials_wait, or by a later
// submit that needs the slot.
struct qldpc_trials_job {
    qldpc_graph *g = nullptr;
    uint32_t *iters_out = nullptr;
    uint8_t *synd_ok_out = nullptr, *keys_match_out = nullptr;
    double *runtime_us_out = nullptr;
    std::vector<int> rcs;           // per device slice (written under that device's trial_mu)
    std::vector<std::string> errs;
};

namespace {

// Wait for a slot's chunk and deliver its results to the job that owns it:
// per trial {iterations, syndromes_match, keys_match} and its share of the
// chunk's window (QKD_LDPC's per-trial window on device, HIP events on the
// slot's stream) in proportion to its own decode span.  dg->trial_mu held.
int harvest_slot(qldpc_graph *g, DeviceGraph *dg, int gi, TrialSlot &t) {
    if (t.nb == 0) return QLDPC_OK;
    qldpc_trials_job *job = t.owner;
    const int nb = t.nb;
    t.nb = 0;
    t.owner = nullptr;
    auto body = [&]() -> int {
        HIP_TRY(hipStreamSynchronize(t.stream));
        int r = split_check(g, dg, t.stream);
        if (r) return r;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, t.ev0, t.ev1));
        if (t.prev_end) {  // (ended before this chunk's decode began: the stream waited for it)
            float mp = 0.f;
            HIP_TRY(hipEventElapsedTime(&mp, t.prev_end, t.ev1));
            if (mp < ms) ms = mp;
            t.prev_end = nullptr;
        }
        const uint64_t *h_clk = t.h_clk.get();
        double span_sum = 0.;
        for (int i = 0; i < nb; ++i) span_sum += (double)(h_clk[2 * i + 1] - h_clk[2 * i]);
        for (int i = 0; i < nb; ++i) {
            job->iters_out[t.f0 + i] = t.h_iters.get()[i];
            job->synd_ok_out[t.f0 + i] = t.h_ok.get()[i];
            job->keys_match_out[t.f0 + i] = t.h_km.get()[i];
            if (job->runtime_us_out) {
                const double span = (double)(h_clk[2 * i + 1] - h_clk[2 * i]);
                job->runtime_us_out[t.f0 + i] =
                    span_sum > 0. ? 1e3 * (double)ms * span / span_sum : 1e3 * (double)ms / nb;
            }
        }
        return QLDPC_OK;
    };
    const int r = body();
    if (r && job->rcs[gi] == QLDPC_OK) {  // the error belongs to the owning job's slice
        job->rcs[gi] = r;
        job->errs[gi] = g_last_error;
    }
    return r;
}

}  // namespace

extern "C" {

int qldpc_run_trials_submit(qldpc_graph *g, const qldpc_rate_plan *plan, const qldpc_params *p, double qber,
                            int32_t count, const uint64_t *seeds, uint64_t seed_add, uint32_t *iters_out,
                            uint8_t *synd_ok_out, uint8_t *keys_match_out, double *runtime_us_out,
                            double *accurate_qber_out, qldpc_trials_job **job_out) {
    if (!job_out) return fail(QLDPC_EINVAL, "job_out is NULL");
    *job_out = nullptr;
    if (!g) return fail(QLDPC_EINVAL, "graph is NULL");
    int rc = check_params(p);
    if (rc) return rc;
    if (count < 0) return fail(QLDPC_EINVAL, "count must be >= 0");
    if (g->devs.empty()) return fail(QLDPC_EINVAL, "graph has no device (host-only)");
    const int n = g->n;
    const uint64_t n_err = (uint64_t)((double)n * qber);
    if (n_err == 0)  // run_trial's own check (src/simulation.cpp:552-553)
        return fail(QLDPC_EINVAL, "Key size '" + std::to_string(n) + "' is too small for QBER.");
    if (n_err > (uint64_t)n) return fail(QLDPC_EINVAL, "QBER must be <= 1");
    const double q_acc = (double)n_err / (double)n;  // inject_errors' return (:922-933)
    if (accurate_qber_out) *accurate_qber_out = q_acc;
    if (count > 0 && (!seeds || !iters_out || !synd_ok_out || !keys_match_out))
        return fail(QLDPC_EINVAL, "NULL host buffer");
    if (plan && plan->n_punct + plan->n_short > n) return fail(QLDPC_EINVAL, "rate plan does not fit the graph");
    const int G = (int)g->devs.size();
    std::unique_ptr<qldpc_trials_job> job(new qldpc_trials_job);
    job->g = g;
    job->iters_out = iters_out;
    job->synd_ok_out = synd_ok_out;
    job->keys_match_out = keys_match_out;
    job->runtime_us_out = runtime_us_out;
    job->rcs.assign(G, QLDPC_OK);
    job->errs.assign(G, std::string());
    if (count == 0) {
        *job_out = job.release();
        return QLDPC_OK;
    }
    const double lp = qldpc_log_p(q_acc);  // log((1 - q) / q) by the host C library (:1043)
    const int n_punct = plan ? plan->n_punct : 0;
    // Bytes of one trial in a pipeline slot (keys, frames, results, generator workspace).
    const size_t per_frame = 4 * (size_t)n + (size_t)g->m + 2 * (size_t)n_punct + 64 +
                             4 * trials_scratch_words(n, n_err, n_punct, 64) / 64;
    // Frames per chunk: a device's whole slice within ~512 MiB of the slot's own
    // buffers (16384 frames at most); longer slices alternate chunks over the
    // two slots.  (The persistent decode holds every CU, so halving a slice buys
    // no overlap: C2, 4096 trials, 2 x 2048 took 22.3 ms, 1 x 4096 21.5 ms;
    // profiles/r04/seam_chunk_ab.txt.)  QLDPC_TRIAL_CHUNK overrides.
    int cap = (int)std::max<size_t>(1, std::min<size_t>(16384, ((size_t)512 << 20) / per_frame));
    if (env_int("QLDPC_TRIAL_CHUNK", 0) > 0) cap = env_int("QLDPC_TRIAL_CHUNK", 0);
    qldpc_trials_job *J = job.get();
    auto work = [&](int gi) {
        DeviceGraph *dg = g->devs[gi].get();
        int32_t lo = 0, hi = 0;
        (void)qldpc_shard_range(count, G, gi, &lo, &hi);
        if (hi <= lo) return;
        auto body = [&]() -> int {
            HIP_TRY(hipSetDevice(dg->device));
            std::lock_guard<std::mutex> lk(dg->trial_mu);
            auto ensure = [&](TrialSlot &t, int nb) -> int {
                if (!t.stream) HIP_TRY(hipStreamCreateWithFlags(t.stream.put(), hipStreamNonBlocking));
                if (!t.ev0) HIP_TRY(hipEventCreate(t.ev0.put()));
                for (Event &e : t.ev_end)
                    if (!e) HIP_TRY(hipEventCreate(e.put()));
                if ((size_t)nb > t.cap || (size_t)std::max(n_punct, 1) > t.cap_punct) {
                    const size_t c = std::max((size_t)nb, t.cap), cp = std::max((size_t)std::max(n_punct, 1), t.cap_punct);
                    int r;
                    if ((r = t.seeds.alloc(c)) || (r = t.clk.alloc(2 * c)) || (r = t.alice.alloc(c * n)) ||
                        (r = t.bob.alloc(c * n)) || (r = t.alice_ext.alloc(c * n)) || (r = t.bits.alloc(c * n)) ||
                        (r = t.synd.alloc(c * (size_t)std::max(g->m, 1))) || (r = t.ok.alloc(c)) ||
                        (r = t.km.alloc(c)) || (r = t.iters.alloc(c)) || (r = t.logp.alloc(c)) ||
                        (r = t.palice.alloc(c * cp)) || (r = t.pbob.alloc(c * cp)))
                        return r;

                    t.cap = 0;
                    if ((r = t.h_iters.alloc(c)) || (r = t.h_ok.alloc(c)) || (r = t.h_km.alloc(c)) ||
                        (r = t.h_clk.alloc(2 * c)) || (r = t.h_seeds.alloc(c)) || (r = t.h_logp.alloc(c)))
                        return r;
                    t.cap = c;
                    t.cap_punct = cp;
                }
                // the generator's workspace also grows with the error count k
                const size_t sw = trials_scratch_words(n, n_err, n_punct, (int)t.cap);
                if (sw > t.tscratch_words) {
                    int r = t.tscratch.alloc(sw);
                    if (r) return r;
                    t.tscratch_words = sw;
                }
                return QLDPC_OK;
            };
            int r = QLDPC_OK;
            for (int f = lo; f < hi && !r;) {
                TrialSlot &t = dg->tslot[dg->next_slot];
                dg->next_slot ^= 1;
                const TrialSlot &o = dg->tslot[dg->next_slot];  // the other slot
                (void)harvest_slot(g, dg, gi, t);  // (a previous chunk, possibly another job's)
                const int nb = std::min(cap, hi - f);
                if ((r = ensure(t, nb))) break;
                auto enqueue = [&]() -> int {
                    // (the slot's pinned inputs are free: its previous chunk was harvested)
                    std::memcpy(t.h_seeds.get(), seeds + f, (size_t)nb * sizeof(uint64_t));
                    std::fill(t.h_logp.get(), t.h_logp.get() + nb, lp);
                    HIP_TRY(hipMemcpyAsync(t.seeds.get(), t.h_seeds.get(), (size_t)nb * sizeof(uint64_t),
                                           hipMemcpyHostToDevice, t.stream));
                    HIP_TRY(hipMemcpyAsync(t.logp.get(), t.h_logp.get(), (size_t)nb * sizeof(double),
                                           hipMemcpyHostToDevice, t.stream));
                    // run_trial's keys (+ QKD_LDPC_RATE_ADAPT's punctured draws), seed = seeds[n] + curr_sim (:743)
                    HIP_TRY(launch_trials(n, n_err, nb, t.seeds.get(), seed_add, t.alice.get(), t.bob.get(),
                                          t.tscratch.get(), n_punct, t.palice.get(), t.pbob.get(), t.stream));
                    // Trial generation, frame build and claim order overlap the
                    // other slot's chunk (the previous chunk, or the previous
                    // combination's under qldpc_run_trials_submit); the decode
                    // waits for it to end, so two decodes never share the CUs
                    // and the chunk's window, started no earlier than that end
                    // (harvest_slot), is its own work.
                    HIP_TRY(hipEventRecord(t.ev0, t.stream));
                    t.ev_i ^= 1;
                    t.ev1 = t.ev_end[t.ev_i];
                    t.prev_end = o.nb > 0 ? o.ev1 : nullptr;
                    int rr = qkd_ldpc_window(g, dg, plan, p, nb, t.alice.get(), t.bob.get(), t.palice.get(),
                                             t.pbob.get(), t.logp.get(), t.alice_ext.get(), nullptr, t.synd.get(),
                                             t.bits.get(), t.iters.get(), t.ok.get(), t.km.get(), t.stream,
                                             t.clk.get(), t.prev_end);
                    if (rr) return rr;
                    HIP_TRY(hipEventRecord(t.ev1, t.stream));
                    HIP_TRY(hipMemcpyAsync(t.h_iters.get(), t.iters.get(), (size_t)nb * sizeof(uint32_t),
                                           hipMemcpyDeviceToHost, t.stream));
                    HIP_TRY(hipMemcpyAsync(t.h_ok.get(), t.ok.get(), (size_t)nb, hipMemcpyDeviceToHost, t.stream));
                    HIP_TRY(hipMemcpyAsync(t.h_km.get(), t.km.get(), (size_t)nb, hipMemcpyDeviceToHost, t.stream));
                    HIP_TRY(hipMemcpyAsync(t.h_clk.get(), t.clk.get(), 2 * (size_t)nb * sizeof(uint64_t),
                                           hipMemcpyDeviceToHost, t.stream));
                    return QLDPC_OK;
                };
                if ((r = enqueue())) {
                    (void)hipStreamSynchronize(t.stream);  // nothing of this chunk stays in flight
                    break;
                }
                t.owner = J;
                t.f0 = f;
                t.nb = nb;
                f += nb;
            }
            if (r) {  // an error: drain this job's chunks in flight on the device
                for (auto &t : dg->tslot)
                    if (t.owner == J) {
                        (void)hipStreamSynchronize(t.stream);
                        t.nb = 0;
                        t.owner = nullptr;
                    }
            }
            return r;
        };
        const int r = body();
        if (r) {
            std::lock_guard<std::mutex> lk(dg->trial_mu);
            if (J->rcs[gi] == QLDPC_OK) {
                J->rcs[gi] = r;
                J->errs[gi] = g_last_error;
            }
        }
    };
    {
        DeviceScope restore;
        if ((rc = restore.save())) return rc;
        if (G == 1) {
            work(0);
        } else {
            std::vector<std::thread> th;
            for (int gi = 0; gi < G; ++gi) th.emplace_back(work, gi);
            for (auto &t : th) t.join();
        }
    }
    *job_out = job.release();
    return QLDPC_OK;
}

int qldpc_run_trials_wait(qldpc_trials_job *job) {
    if (!job) return fail(QLDPC_EINVAL, "job is NULL");
    std::unique_ptr<qldpc_trials_job> own(job);
    qldpc_graph *g = job->g;
    {
        DeviceScope restore;
        if (int rc = restore.save()) return rc;
        for (int gi = 0; gi < (int)g->devs.size(); ++gi) {
            DeviceGraph *dg = g->devs[gi].get();
            std::lock_guard<std::mutex> lk(dg->trial_mu);
            if (hipSetDevice(dg->device) != hipSuccess) continue;
            for (auto &t : dg->tslot)
                if (t.owner == job) (void)harvest_slot(g, dg, gi, t);
        }
    }
    for (int gi = 0; gi < (int)job->rcs.size(); ++gi)
        if (job->rcs[gi]) return fail(job->rcs[gi], job->errs[gi]);
    return QLDPC_OK;
}

int qldpc_run_trials(qldpc_graph *g, const qldpc_rate_plan *plan, const qldpc_params *p, double qber, int32_t count,
                     const uint64_t *seeds, uint64_t seed_add, uint32_t *iters_out, uint8_t *synd_ok_out,
                     uint8_t *keys_match_out, double *runtime_us_out, double *accurate_qber_out) {
    qldpc_trials_job *job = nullptr;
    const int rc = qldpc_run_trials_submit(g, plan, p, qber, count, seeds, seed_add, iters_out, synd_ok_out,
                                           keys_match_out, runtime_us_out, accurate_qber_out, &job);
    if (rc) return rc;
    return qldpc_run_trials_wait(job);
}

}  // extern "C"
