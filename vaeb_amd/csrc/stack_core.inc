// stack_core.inc -- the host core of the layer-stack engine: what a handle on the layer-stack
// kernels (ae_mlp.hpp) holds and does whatever its network, embedded by vaeb_ae (engine_ae.inc) and
// vaeb_clf (engine_clf.inc).  Included by vaeb_hip.hip before the two.  A handle adds its layers
// (AeLayer, laid out by core_place), its buffers and its own kernels; through the core go
//   create / destroy    core_open (device, stream, theta, state slot 0) ... core_ready (index list,
//                       step values, the one device synchronise) | core_close; the handle's own
//                       type is deleted by its engine file
//   launches            core_fwd_layer (PAeFwd F_ACT | F_LINEAR; ae_fwd_args fills the fields every
//                       forward shares), core_bwd_layer (PAeBwdT, then the heads' core_wgrad),
//                       core_wgrad (PAeWgradT<RULE, MASK>)
//   the update rule     core_set_optimizer, core_opt_state, core_set_opt_step; core_xfer (an arena)
//   training            core_train_many: checks, index upload, a step per batch, the values, one sync
//   host rows           core_chunks (one or two matrices in max_batch chunks), core_sum_to_host

// One affine map of theta: W [K x N] at theta + oW, b [N] at theta + ob.
struct AeLayer { int K, N; int64_t oW, ob; };

// Rows of a row-major matrix p [rows x width]: row m of a launch is p[m], or p[idx[m]] when
// idx is set (the dataset rows of a step; the chunk rows the stacked sample planes observe).
struct AeRows { const float* p; int rows; const int* idx; };

struct StackCore {
    hipStream_t s = nullptr;
    int64_t P = 0;
    DevOwner mem;                     // every device allocation; released by core_close
    // acc is slot 0 of the update rule's state, acc2 slot 1 (allocated when a two-slot rule is
    // first set)
    float *theta = nullptr, *acc = nullptr, *acc2 = nullptr;
    // the update rule ({ADAGRAD, eta, 0, 0, 1e-6} from create): launch arguments; opt_t counts the
    // optimiser steps taken (Adam's t - 1 of the next)
    vaeb_ae_optimizer opt{};
    int64_t opt_t = 0;
    int* idx = nullptr;               // device index list (epoch capacity)
    float* outs = nullptr;            // the step values of a training call
    int64_t idx_cap = 0, outs_cap = 0;
    double* esum = nullptr;           // one chunk's fp64 sum (core_sum_to_host)
    int act = 0, max_batch = 0;       // the handle's config, as the launches and the chunk loop read it
};

namespace {

// theta order within a group of n layers: the group's W's, then its b's, from offset *o on.
void core_place(int64_t* o, AeLayer* l, int n) {
    for (int i = 0; i < n; ++i) { l[i].oW = *o; *o += (int64_t)l[i].K * l[i].N; }
    for (int i = 0; i < n; ++i) { l[i].ob = *o; *o += l[i].N; }
}

int core_reserve(StackCore* k, int64_t n_idx, int64_t n_out) {
    if (int rc = k->mem.grow(&k->idx, &k->idx_cap, n_idx)) return rc;
    return k->mem.grow(&k->outs, &k->outs_cap, n_out);
}

// The destroy body: the enqueued work, every device buffer, the stream.  The caller deletes the handle.
void core_close(StackCore* k) {
    if (k->s) hipStreamSynchronize(k->s);
    k->mem.release_all();
    if (k->s) hipStreamDestroy(k->s);
    k->s = nullptr;
}

// A fresh handle (P set) on its device: the stream, theta and state slot 0, AdaGrad at eta.  A
// failure closes the core; the caller deletes the handle.
int core_open(StackCore* k, int device, float eta, int act, int max_batch) {
    k->opt = vaeb_ae_optimizer{VAEB_AE_RULE_ADAGRAD, eta, 0.f, 0.f, 1e-6f};
    k->act = act; k->max_batch = max_batch;
    int rc = 0;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&k->s, hipStreamNonBlocking) != hipSuccess)
        rc = fail(VAEB_ERR_HIP, "device / stream init failed");
    rc = rc ? rc : k->mem.alloc(&k->theta, k->P);
    rc = rc ? rc : k->mem.alloc(&k->acc, k->P);
    if (rc) core_close(k);
    return rc;
}

// The end of a create whose allocations returned rc: the index list and the step values of one
// batch, the final device synchronise; a failure closes the core and the caller deletes the handle.
int core_ready(StackCore* k, int rc) {
    rc = rc ? rc : core_reserve(k, k->max_batch, 1);
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(VAEB_ERR_HIP, "device init failed");
    if (rc) core_close(k);
    return rc;
}

// ------------------------------------------------------------------ launches
// The arguments every forward launch of layer l shares: M rows of in through W and b of arena th.
template <class P>
P ae_fwd_args(const float* th, const AeLayer& l, const AeRows& in, int M) {
    P p{};
    p.M = M; p.N = l.N; p.K = l.K;
    p.in = in.p; p.ldin = l.K; p.in_rows = in.rows; p.idx = in.idx;
    p.W = th + l.oW; p.b = th + l.ob;
    return p;
}

// out = f(in W + b) (ae::F_ACT) or in W + b (ae::F_LINEAR) under the arena th (theta, or a dropout
// classifier's masked copy)
int core_fwd_layer(StackCore* k, const float* th, const AeLayer& l, const AeRows& in, int M, int mode, float* out) {
    ae::PAeFwd p = ae_fwd_args<ae::PAeFwd>(th, l, in, M);
    p.mode = mode; p.act = k->act; p.out = out;
    launch_bigk<1>(k->s, p);
    CHECK_LAUNCH();
    return 0;
}

// A rule's own launch arguments into its parameter block (nothing into AdaGrad's: the overload is
// chosen by the block's base).  Adam's bias corrections are those of the step being enqueued,
// t = opt_t + 1, formed in double: every step of a training call carries its own.
bool ae_two_slot(int rule) { return rule == VAEB_AE_RULE_ADADELTA || rule == VAEB_AE_RULE_ADAM; }
void ae_put_rule(const StackCore*, ae::AeRuleArgs<ae::RULE_ADAGRAD>&) {}
void ae_put_rule(const StackCore* k, ae::AeRuleArgs<ae::RULE_SGA>& q) { q.mu = k->opt.beta1; }
void ae_put_rule(const StackCore* k, ae::AeRuleArgs<ae::RULE_ADADELTA>& q) {
    q.state1 = k->acc2; q.rho = k->opt.beta1; q.eps = k->opt.eps;
}
void ae_put_rule(const StackCore* k, ae::AeRuleArgs<ae::RULE_ADAM>& q) {
    const double t = (double)(k->opt_t + 1);
    q.state1 = k->acc2; q.b1 = k->opt.beta1; q.b2 = k->opt.beta2; q.eps = k->opt.eps;
    q.bc1 = (float)(1.0 - std::pow((double)k->opt.beta1, t));
    q.bc2 = (float)(1.0 - std::pow((double)k->opt.beta2, t));
}

// One weight-gradient + update launch for layer l from its input in (gathered through in.idx for
// the first layer) and its output delta over M rows, in the instantiation of the handle's rule;
// mask (a dropout step's byte mask) selects the MASK instantiations, nullptr the unmasked ones.
// inv_s2: the prior's 1 / s2, or 0 without one.  The one place that launches the update.
int core_wgrad(StackCore* k, const AeLayer& l, const AeRows& in, const float* dout, int M, float inv_s2,
               const uint8_t* mask) {
    auto launch = [&](auto p) {
        p.M = l.K + 1; p.N = l.N; p.K = M;
        p.in = in.p; p.ldin = l.K; p.in_rows = in.rows; p.idx = in.idx; p.Kin = l.K;
        p.dout = dout;
        p.theta = k->theta; p.accum = k->acc; p.offW = l.oW; p.offb = l.ob;
        p.eta = k->opt.eta; p.inv_s2 = inv_s2;
        ae_put_rule(k, p);
        if constexpr (std::is_base_of_v<ae::AeMaskArgs<true>, decltype(p)>) p.mask = mask;
        launch_bigk<1>(k->s, p);
    };
    auto rule = [&](auto r) {
        if (mask) launch(ae::PAeWgradT<decltype(r)::value, true>{});
        else launch(ae::PAeWgradT<decltype(r)::value>{});
    };
    switch (k->opt.rule) {
    case VAEB_AE_RULE_ADAGRAD: rule(std::integral_constant<int, ae::RULE_ADAGRAD>{}); break;
    case VAEB_AE_RULE_SGA: rule(std::integral_constant<int, ae::RULE_SGA>{}); break;
    case VAEB_AE_RULE_ADADELTA: rule(std::integral_constant<int, ae::RULE_ADADELTA>{}); break;
    case VAEB_AE_RULE_ADAM: rule(std::integral_constant<int, ae::RULE_ADAM>{}); break;
    default: return fail(VAEB_ERR_STATE, "unknown update rule %d", k->opt.rule);
    }
    CHECK_LAUNCH();
    return 0;
}

// Backward through one layer of nh (1 or 2) heads l[] with the pre-activation deltas d[] on the
// input `in` over M rows: the data gradient [d0 | d1] [W0 | W1]^T, then mode, into din with the
// old weights of arena th (din == nullptr: none, no data gradient into x), followed by each head's
// update.  PBwd is the PAeBwdT instantiation; fill(p) adds the caller's own fields to the block
// before the launch (the latent modes' buffers, the sample weights, the prior; nothing for B_DACT).
// This order is load-bearing (ae_mlp.hpp: every weight is updated only after the last kernel of
// the step that reads it), and it exists here only.
template <class PBwd, class Fill>
int core_bwd_layer(StackCore* k, const float* th, const AeLayer* l, float* const* d, int nh, const AeRows& in, int M,
                   int mode, float* din, float inv_s2, const uint8_t* mask, Fill fill) {
    if (din) {
        PBwd p{};
        p.M = M; p.N = l[0].K; p.K = nh * l[0].N;
        p.dout = d[0]; p.K1 = l[0].N; p.W = th + l[0].oW;
        if (nh == 2) { p.dout2 = d[1]; p.W2 = th + l[1].oW; }
        p.h = in.p; p.mode = mode; p.act = k->act; p.din = din;
        fill(p);
        launch_bigk<1>(k->s, p);
        CHECK_LAUNCH();
    }
    for (int j = 0; j < nh; ++j)
        if (int rc = core_wgrad(k, l[j], in, d[j], M, inv_s2, mask)) return rc;
    return 0;
}

// ------------------------------------------------------------------ the update rule
// Why a vaeb_ae_optimizer is not valid, or nullptr (the rules of vaeb_ae_set_optimizer).
const char* ae_opt_why(const vaeb_ae_optimizer* o) {
    auto unit = [](float b) { return b >= 0.f && b < 1.f; };   // NaN fails
    if (!(o->eta > 0.f) || !std::isfinite(o->eta)) return "eta must be finite and > 0";
    switch (o->rule) {
    case VAEB_AE_RULE_ADAGRAD:
        if (o->eps != 1e-6f) return "AdaGrad's eps is 1e-6 (the kernel's literal)";
        if (o->beta1 != 0.f || o->beta2 != 0.f) return "AdaGrad uses no beta: beta1 and beta2 must be 0";
        return nullptr;
    case VAEB_AE_RULE_SGA:
        if (!unit(o->beta1)) return "the momentum (beta1) must be in [0, 1)";
        if (o->beta2 != 0.f || o->eps != 0.f) return "gradient ascent uses beta1 alone: beta2 and eps must be 0";
        return nullptr;
    case VAEB_AE_RULE_ADADELTA:
        if (!unit(o->beta1) || o->beta1 == 0.f) return "rho (beta1) must be in (0, 1)";
        if (!(o->eps > 0.f) || !std::isfinite(o->eps)) return "eps must be finite and > 0";
        if (o->beta2 != 0.f) return "AdaDelta uses no beta2: it must be 0";
        return nullptr;
    case VAEB_AE_RULE_ADAM:
        if (!unit(o->beta1) || !unit(o->beta2)) return "beta1 and beta2 must be in [0, 1)";
        if (!(o->eps > 0.f) || !std::isfinite(o->eps)) return "eps must be finite and > 0";
        return nullptr;
    }
    return "rule must be VAEB_AE_RULE_ADAGRAD | _SGA | _ADADELTA | _ADAM";
}

int core_num_params(const StackCore* k, int64_t* n) {
    if (!k || !n) return fail(VAEB_ERR_ARG, "null argument");
    *n = k->P;
    return 0;
}

// set (hin) or get (hout) of a P-element arena dev of the handle
int core_xfer(StackCore* k, float* dev, const float* hin, float* hout, int64_t n) {
    if (!k || (!hin && !hout)) return fail(VAEB_ERR_ARG, "null argument");
    if (n != k->P) return fail(VAEB_ERR_ARG, "size mismatch: got %lld, expected %lld", (long long)n, (long long)k->P);
    HIP_TRY(hipStreamSynchronize(k->s));
    if (hin) HIP_TRY(hipMemcpy(dev, hin, sizeof(float) * n, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemcpy(hout, dev, sizeof(float) * n, hipMemcpyDeviceToHost));
    return 0;
}

// vaeb_ae_set_optimizer's and vaeb_clf_set_optimizer's body.  The fields a rule does not use are 0
// (AdaGrad's eps: the kernel's literal 1e-6).
int core_set_optimizer(StackCore* k, const vaeb_ae_optimizer* o) {
    if (!k || !o) return fail(VAEB_ERR_ARG, "null argument");
    const char* why = ae_opt_why(o);
    if (why)
        return fail(VAEB_ERR_ARG, "optimizer {rule %d, eta %g, beta1 %g, beta2 %g, eps %g}: %s", o->rule, (double)o->eta,
                    (double)o->beta1, (double)o->beta2, (double)o->eps, why);
    if (o->rule != k->opt.rule) {   // another rule: its state starts from zero, after the enqueued steps
        if (ae_two_slot(o->rule))
            if (int rc = k->mem.lazy(&k->acc2, k->P)) return rc;
        HIP_TRY(hipMemsetAsync(k->acc, 0, sizeof(float) * (size_t)k->P, k->s));
        if (k->acc2) HIP_TRY(hipMemsetAsync(k->acc2, 0, sizeof(float) * (size_t)k->P, k->s));
        k->opt_t = 0;
    }
    k->opt = *o;   // launch arguments: the enqueued steps keep theirs
    return 0;
}

int core_get_optimizer(StackCore* k, vaeb_ae_optimizer* o) {
    if (!k || !o) return fail(VAEB_ERR_ARG, "null argument");
    *o = k->opt;
    return 0;
}

// set / get of state slot `slot` (hin or hout set)
int core_opt_state(StackCore* k, int32_t slot, const float* hin, float* hout, int64_t n) {
    if (!k || (!hin && !hout)) return fail(VAEB_ERR_ARG, "null argument");
    const bool two = ae_two_slot(k->opt.rule);
    if (slot == 0 || (slot == 1 && two)) return core_xfer(k, slot ? k->acc2 : k->acc, hin, hout, n);
    return fail(VAEB_ERR_ARG, "optimizer state slot %d: rule %d has slot 0%s", slot, k->opt.rule,
                two ? " and slot 1" : " only");
}

int core_set_opt_step(StackCore* k, int64_t t) {
    if (!k) return fail(VAEB_ERR_ARG, "null argument");
    if (t < 0) return fail(VAEB_ERR_ARG, "optimizer step %lld < 0", (long long)t);
    k->opt_t = t;
    return 0;
}

int core_get_opt_step(StackCore* k, int64_t* t) {
    if (!k || !t) return fail(VAEB_ERR_ARG, "null argument");
    *t = k->opt_t;
    return 0;
}

// ------------------------------------------------------------------ training
// The n indices of a call against the resident rows data [nrows x ...] (set_data: the call that
// uploads them).
int core_check_idx(const float* data, int64_t nrows, const char* set_data, const int32_t* idx, int32_t n) {
    if (!data) return fail(VAEB_ERR_STATE, "%s has not been called", set_data);
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= nrows)
            return fail(VAEB_ERR_ARG, "row index %d out of range [0, %lld)", idx[i], (long long)nrows);
    return 0;
}

// train_many: the checks every handle shares, then the handle's own (more()), the index list to
// the device, step(idx, m, slot, lb, n) per batch of m rows at offset lb, the values to out and
// the call's one stream synchronise.
template <class More, class Step>
int core_train_many(StackCore* k, const float* data, int64_t nrows, const char* set_data, const int32_t* idx, int32_t n,
                    int32_t batch, float* out, More more, Step step) {
    if (!k || !idx || !out || n <= 0 || batch <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (batch > k->max_batch) return fail(VAEB_ERR_ARG, "batch %d > max_batch %d", batch, k->max_batch);
    if (int rc = core_check_idx(data, nrows, set_data, idx, n)) return rc;
    if (int rc = more()) return rc;
    const int nb = cdiv(n, batch);
    if (int rc = core_reserve(k, n, nb)) return rc;
    HIP_TRY(hipMemcpyAsync(k->idx, idx, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, k->s));
    for (int j = 0; j < nb; ++j) {
        const int lb = j * batch, m = std::min(batch, n - lb);
        if (int rc = step(k->idx + lb, m, j, lb, n)) return rc;
    }
    HIP_TRY(hipMemcpyAsync(out, k->outs, sizeof(float) * (size_t)nb, hipMemcpyDeviceToHost, k->s));
    HIP_TRY(hipStreamSynchronize(k->s));
    return 0;
}

// ------------------------------------------------------------------ calls over host rows
// Walks the n rows of the host matrix x [n x wx] (and of y [n x wy] when set) in chunks of at most
// max_batch rows: uploads a chunk to xin (yin), then body(r0, rows).  The body ends in the chunk's
// one stream synchronise.
template <class Body>
int core_chunks(StackCore* k, int64_t n, const float* x, int wx, float* xin, const float* y, int wy, float* yin,
                Body body) {
    const int64_t B = k->max_batch;
    for (int64_t r0 = 0; r0 < n; r0 += B) {
        const int rows = (int)std::min<int64_t>(B, n - r0);
        HIP_TRY(hipMemcpyAsync(xin, x + r0 * wx, sizeof(float) * (size_t)rows * wx, hipMemcpyHostToDevice, k->s));
        if (y) HIP_TRY(hipMemcpyAsync(yin, y + r0 * wy, sizeof(float) * (size_t)rows * wy, hipMemcpyHostToDevice, k->s));
        if (int rc = body(r0, rows)) return rc;
    }
    return 0;
}

// The fixed-order fp64 sum of the chunk's row values v [rows] -> esum (v == nullptr: a kernel of
// the body has written esum already), added to *total on the host; the rows themselves to
// out_rows when that is set.  Ends in the chunk's one stream synchronise.
int core_sum_to_host(StackCore* k, const float* v, int rows, double* total, float* out_rows = nullptr) {
    if (v) {
        HIP_TRY(hipMemsetAsync(k->esum, 0, sizeof(double), k->s));
        hipLaunchKernelGGL(iw_sum_kernel, dim3(1), dim3(256), 0, k->s, v, (int64_t)rows, k->esum);
        CHECK_LAUNCH();
    }
    double part = 0.0;
    HIP_TRY(hipMemcpyAsync(&part, k->esum, sizeof(double), hipMemcpyDeviceToHost, k->s));
    if (out_rows) HIP_TRY(hipMemcpyAsync(out_rows, v, sizeof(float) * (size_t)rows, hipMemcpyDeviceToHost, k->s));
    HIP_TRY(hipStreamSynchronize(k->s));
    *total += part;
    return 0;
}

}  // namespace
