// dp_buckets.inc -- the data-parallel gradient buckets: included once by vaeb_hip.hip inside its
// anonymous namespace, used by both engines' training steps and by vaeb_dp_plan /
// vaeb_dp_rank_update.
//
// Arena order W3 W4 W5 W1 W2 [W6] b3 b4 b5 b1 b2 [b6] | SGVB.  Bucket A = W2 [| W6] is final
// once the dW2 (| dW6) launch has run, early in the backward; bucket B = the rest plus the
// SGVB slot, final after the last weight-gradient launch.  Unprofiled steps fork bucket A's
// all-reduce and Adagrad onto s2, where they overlap the remaining backward launches; s
// then waits for bucket A's all-reduce (RCCL calls on one communicator stay serialised, in
// the same order on every rank), reduces bucket B itself, runs its Adagrad and waits for
// bucket A's Adagrad.  Only the fork sits on s2's queue: the critical path on s keeps its
// own queue, and both waits are normally satisfied by the time s reaches them.  Profiled
// steps run one all-reduce and one optimizer launch on s (per-kernel timing).
// The fork costs ~18 us per step on the fp32 engine's 58-us MNIST step at world 1 (hipGraph
// with a second branch; 78 vs 60 us) -- more than a 1.6-MB bucket's all-reduce can hide --
// so it is the bf16 engine's default only, where bucket A is 34 MB (config 5) and its
// Adagrad alone (37 us) pays for the fork already at world 1 (933 vs ~940 us).
// Sharded form (vaeb_ctx::dp_shard, world > 1; VERDICT r3): instead of all-reducing the
// whole bucket and running the replicated Adagrad over all of it on every rank, each rank
// reduce-scatters the bucket, updates ITS 1/W shard (prior + Adagrad; bf16: + shadow), and the
// shards of theta' are all-gathered: the same xGMI bytes as the all-reduce (a ring all-reduce
// is a reduce-scatter + all-gather), the optimizer stream per rank W times shorter, and every
// replica bitwise identical (theta' comes from one owner).  Shards are 64-element aligned; the
// remainder of each run (< 64 W elements, and the SGVB slot) is all-reduced and updated on
// every rank.  The arena is always partitioned into the same three runs -- B0 = [0, W2),
// A = [W2, b3) (W2 | W6), B1 = [b3, P) -- so an element's owner (and its Adagrad state, kept
// on the owner only) is the same whichever bucket form a step takes.
struct DpBucket {
    int nrun;
    int64_t lo[3], n[3];
    bool slot;   // + grad[P] (the SGVB), right after the run that ends at P (the last one)
};
DpBucket dp_bucket_a_runs(const vaeb_ctx* c) {
    const int64_t w2 = c->off[c->sl.W2], b3 = c->off[c->sl.b3];
    return DpBucket{1, {w2, 0, 0}, {b3 - w2, 0, 0}, false};
}
DpBucket dp_bucket_b_runs(const vaeb_ctx* c) {
    const int64_t w2 = c->off[c->sl.W2], b3 = c->off[c->sl.b3];
    return DpBucket{2, {0, b3, 0}, {w2, c->P - b3, 0}, true};
}
DpBucket dp_bucket_all_runs(const vaeb_ctx* c) {
    const int64_t w2 = c->off[c->sl.W2], b3 = c->off[c->sl.b3];
    return DpBucket{3, {0, w2, b3}, {w2, b3 - w2, c->P - b3}, true};
}
// elements per rank of a run of n (0: the run is all-reduced and updated everywhere)
int64_t dp_shard_len(const vaeb_ctx* c, int64_t n) { return c->dp_shard ? (n / c->world) & ~(int64_t)63 : 0; }
// what this rank's optimizer launch updates: each run's own shard and its replicated remainder
DpRange dp_opt_range(const vaeb_ctx* c, const DpBucket& bk) {
    DpRange r{};
    int k = 0;
    for (int j = 0; j < bk.nrun; ++j) {
        const int64_t S = dp_shard_len(c, bk.n[j]), tail = bk.n[j] - c->world * S;
        if (S) { r.lo[k] = bk.lo[j] + c->rank * S; r.n[k++] = S; }
        if (tail) { r.lo[k] = bk.lo[j] + c->world * S; r.n[k++] = tail; }
    }
    r.book = bk.slot ? 1 : 0;
    return r;
}
// the elements of the bucket other ranks updated (their shards): the bf16 shadow fix
DpRange dp_foreign_range(const vaeb_ctx* c, const DpBucket& bk) {
    DpRange r{};
    int k = 0;
    for (int j = 0; j < bk.nrun; ++j) {
        const int64_t S = dp_shard_len(c, bk.n[j]);
        if (!S) continue;
        if (c->rank > 0) { r.lo[k] = bk.lo[j]; r.n[k++] = c->rank * S; }
        if (c->rank < c->world - 1) { r.lo[k] = bk.lo[j] + (c->rank + 1) * S; r.n[k++] = (c->world - c->rank - 1) * S; }
    }
    return r;
}

// The fp32 engine's DP optimizer launch over range r (prior + Adagrad; r.book: also the SGVB
// bookkeeping): the step's dp_opt, and what vaeb_dp_rank_update runs for one emulated rank.
int dp_opt_launch(vaeb_ctx* c, hipStream_t st, const OptArgs& o, const DpRange& r, const ElboArgs& e) {
    int64_t n = 0;
    for (int k = 0; k < kDpRuns; ++k) n += r.n[k];
    // (sharded: a 1/W share of the arena; the grid scales down with it)
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(r.book ? 512 : 256, cdiv(n, 256 * 8)));
    hipLaunchKernelGGL(adagrad_kernel, dim3(nb), dim3(256), 0, st, o, c->P, r, e);
    CHECK_LAUNCH();
    return 0;
}

int nccl_ok(ncclResult_t r, const char* what) {
    return r == ncclSuccess ? 0 : fail(VAEB_ERR_COMM, "%s: %s", what, ncclGetErrorString(r));
}
int nccl_sum(vaeb_ctx* c, float* p, int64_t n, hipStream_t st) {
    return nccl_ok(ncclAllReduce(p, p, (size_t)n, ncclFloat, ncclSum, c->comm, st), "ncclAllReduce");
}

// One bucket on stream st: the reduction (reduce-scatter of each run's shards + all-reduce of
// the remainders and the slot, one RCCL group), this rank's optimizer launch, then (sharded)
// the all-gather of theta' shards and fix(st, foreign range) for the bf16 shadow.  comm_done
// (if any) is recorded after the bucket's last collective: another stream's collectives wait
// for it (RCCL calls on one communicator stay serialised, in the same order on every rank).
template <class Opt, class Fix>
int dp_reduce_update(vaeb_ctx* c, hipStream_t st, const DpBucket& bk, float* theta_out, Opt opt, Fix fix,
                     hipEvent_t comm_done, Prof* pr = nullptr, KernelId opt_mark = K_END) {
    const int W = c->world, rk = c->rank;
    bool sharded = false;
    if (pr) pr->mark(K_ALLREDUCE);
    for (int rep = 0; rep < (pr ? pr->reps : 1); ++rep) {
        if (int rc = nccl_ok(ncclGroupStart(), "ncclGroupStart")) return rc;
        int rc = 0;
        for (int j = 0; j < bk.nrun && !rc; ++j) {
            const int64_t S = dp_shard_len(c, bk.n[j]);
            const int64_t tail = bk.n[j] - W * S + ((bk.slot && j == bk.nrun - 1) ? 1 : 0);
            float* g = c->grad + bk.lo[j];
            if (S) {
                sharded = true;
                rc = nccl_ok(ncclReduceScatter(g, g + rk * S, (size_t)S, ncclFloat, ncclSum, c->comm, st),
                             "ncclReduceScatter");
            }
            if (!rc && tail) rc = nccl_sum(c, g + W * S, tail, st);
        }
        const int re = nccl_ok(ncclGroupEnd(), "ncclGroupEnd");
        if (rc) return rc;
        if (re) return re;
    }
    if (comm_done && !sharded) HIP_TRY(hipEventRecord(comm_done, st));
    if (pr) pr->mark(opt_mark);
    for (int rep = 0; rep < (pr ? pr->reps : 1); ++rep)
        if (int rc = opt(st, dp_opt_range(c, bk))) return rc;
    if (!sharded) return 0;
    if (int rc = nccl_ok(ncclGroupStart(), "ncclGroupStart")) return rc;
    int rc = 0;
    for (int j = 0; j < bk.nrun && !rc; ++j) {
        const int64_t S = dp_shard_len(c, bk.n[j]);
        float* t = theta_out + bk.lo[j];
        if (S) rc = nccl_ok(ncclAllGather(t + rk * S, t, (size_t)S, ncclFloat, c->comm, st), "ncclAllGather");
    }
    const int re = nccl_ok(ncclGroupEnd(), "ncclGroupEnd");
    if (rc) return rc;
    if (re) return re;
    if (comm_done) HIP_TRY(hipEventRecord(comm_done, st));
    return fix(st, dp_foreign_range(c, bk));
}

// Sharded Adagrad keeps each element's accumulator on its owner only: gather the shards before
// the host reads the state (vaeb_get_adagrad_state, vaeb_checkpoint_save; every rank calls it).
int dp_gather_acc(vaeb_ctx* c) {
    if (!c->comm || !c->dp_shard) return 0;
    const DpBucket bk = dp_bucket_all_runs(c);
    if (int rc = nccl_ok(ncclGroupStart(), "ncclGroupStart")) return rc;
    int rc = 0;
    for (int j = 0; j < bk.nrun && !rc; ++j) {
        const int64_t S = dp_shard_len(c, bk.n[j]);
        float* t = c->acc + bk.lo[j];
        if (S) rc = nccl_ok(ncclAllGather(t + c->rank * S, t, (size_t)S, ncclFloat, c->comm, c->s), "ncclAllGather");
    }
    const int re = nccl_ok(ncclGroupEnd(), "ncclGroupEnd");
    if (rc) return rc;
    if (re) return re;
    HIP_TRY(hipStreamSynchronize(c->s));
    return 0;
}

// after the dW2 (| dW6) launch: opt(stream, range) enqueues the optimizer over a range,
// fix(stream, range) the bf16 shadow of other ranks' shards (fp32: nothing)
template <class Opt, class Fix>
int dp_bucket_a(vaeb_ctx* c, const Prof& pr, float* theta_out, Opt opt, Fix fix) {
    if (pr.on || !c->dp_overlap) return 0;
    HIP_TRY(hipEventRecord(c->dp_ev[0], c->s));
    HIP_TRY(hipStreamWaitEvent(c->s2, c->dp_ev[0], 0));
    if (int rc = dp_reduce_update(c, c->s2, dp_bucket_a_runs(c), theta_out, opt, fix, c->dp_ev[1])) return rc;
    HIP_TRY(hipEventRecord(c->dp_ev[2], c->s2));
    return 0;
}

// after the last weight-gradient launch (the SGVB slot written)
template <class Opt, class Fix>
int dp_bucket_b(vaeb_ctx* c, Prof& pr, KernelId opt_mark, float* theta_out, Opt opt, Fix fix) {
    if (pr.on || !c->dp_overlap)
        return dp_reduce_update(c, c->s, dp_bucket_all_runs(c), theta_out, opt, fix, nullptr, pr.on ? &pr : nullptr,
                                opt_mark);
    HIP_TRY(hipStreamWaitEvent(c->s, c->dp_ev[1], 0));
    if (int rc = dp_reduce_update(c, c->s, dp_bucket_b_runs(c), theta_out, opt, fix, nullptr)) return rc;
    HIP_TRY(hipStreamWaitEvent(c->s, c->dp_ev[2], 0));
    return 0;
}
