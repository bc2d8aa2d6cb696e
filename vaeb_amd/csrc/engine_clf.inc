// engine_clf.inc -- the softmax MLP classifier (include/vaeb_hip.h vaeb_clf_*) on the layer-stack
// kernels (ae_mlp.hpp) and clf_softmax.hpp.  Included by vaeb_hip.hip after stack_core.inc: vaeb_clf
// is a StackCore, as vaeb_ae is, and every launch of the layer-stack kernels, the update rule's
// calls, the training driver, the chunk loop and the chunk sum are the core's.  Each call and the
// helper sequence it runs:
//   vaeb_clf_train(_many)  core_train_many, per batch clf_step: (dropout: clf_mask, training domain) |
//                          clf_forward (core_fwd_layer per layer) | clf_softmax (value + P + deltas) |
//                          ae_loglik_kernel (the sum) | per layer, top down, clf_bwd_layer =
//                          core_bwd_layer, one head, B_DACT
//   vaeb_clf_predict       clf_chunks: clf_probs = per draw (clf_mask, evaluation domain) |
//                          clf_forward | clf_softmax (predictions; draws >= 1: the running mean)
//   vaeb_clf_loglik        clf_chunks: clf_forward | clf_softmax (value) | core_sum_to_host
//   vaeb_clf_accuracy      clf_chunks: clf_probs | clf_hit_kernel | clf_count_kernel
//   vaeb_clf_draw_mask     clf_mask (mask bytes only)
// A dropout context's forward and data-backward launches read the masked arena thm where a MAP
// context's read theta: a pointer, no other kernel.  Its weight-gradient launch is the MASK
// instantiation PAeWgradT<RULE, true> (core_wgrad given the mask), which updates the real theta.

struct vaeb_clf : StackCore {
    vaeb_clf_config c{};
    AeLayer hid[VAEB_AE_MAX_LAYERS] = {}, out{};   // Din -> Dh..., then Dh[n - 1] -> Dout
    float* thm = nullptr;                          // dropout: theta * m of the last draw
    uint8_t* mask = nullptr;                       // dropout: m of the last draw [P]
    float *x = nullptr, *y = nullptr;              // resident Xtr, Ytr
    int64_t nrows = 0;
    float *H[VAEB_AE_MAX_LAYERS + 1] = {}, *dH[VAEB_AE_MAX_LAYERS + 1] = {};   // H[0], dH[0] unused
    float *A = nullptr, *Pr = nullptr, *dA = nullptr, *rowval = nullptr;       // logits, P, deltas, row values
    float *Pacc = nullptr, *xin = nullptr, *yin = nullptr;                     // MC mean; a chunk's host rows
    int* hit = nullptr;
    long long* count = nullptr;
    uint64_t seed = 0;
    int64_t step = 0;                              // Philox step counter of the dropout draws
    uint64_t T = 0;                                // keep iff word < T: floor(keep * 2^32)
};

namespace {

bool clf_dropout(const vaeb_clf* c) { return c->c.dropout != 0; }

// m of (step, domain) into mask and theta * m into thm (either may be nullptr).
int clf_mask(vaeb_clf* c, int64_t step, uint32_t domain, float* thm, uint8_t* mask) {
    clf::MaskArgs q{};
    q.theta = c->theta; q.thm = thm; q.mask = mask; q.P = c->P;
    q.seed = c->seed; q.step = step; q.domain = domain; q.T = c->T;
    hipLaunchKernelGGL(clf::clf_mask_kernel, dim3(cdiv(cdiv(c->P, 4), 256)), dim3(256), 0, c->s, q);
    CHECK_LAUNCH();
    return 0;
}

// The arena the network reads for evaluation draw `draw` (-1: theta itself).
int clf_eval_weights(vaeb_clf* c, int draw, const float** th) {
    *th = c->theta;
    if (draw < 0) return 0;
    *th = c->thm;
    return clf_mask(c, c->step, 1u | ((uint32_t)(draw + 1) << 1), c->thm, nullptr);
}

// Hidden activations H[1..n] and the logits A of the M rows of x under the arena th.
int clf_forward(vaeb_clf* c, const float* th, const AeRows& x, int M) {
    const int nh = c->c.n_hidden;
    for (int i = 0; i < nh; ++i)
        if (int rc = core_fwd_layer(c, th, c->hid[i], i == 0 ? x : AeRows{c->H[i], M, nullptr}, M, ae::F_ACT, c->H[i + 1]))
            return rc;
    return core_fwd_layer(c, th, c->out, AeRows{c->H[nh], M, nullptr}, M, ae::F_LINEAR, c->A);
}

// The softmax output on the logits of M rows.  y.p == nullptr: predictions only.
int clf_softmax(vaeb_clf* c, int M, const AeRows& y, float* P, float* d, float* Pacc = nullptr, int l = 0, int L = 1) {
    clf::SoftmaxArgs q{};
    q.a = c->A; q.M = M; q.D = c->c.Dout;
    q.Y = y.p; q.yidx = y.idx; q.loss = c->c.loss;
    q.P = P; q.d = d; q.rowval = c->rowval;
    q.Pacc = Pacc; q.first = l == 0; q.last = l == L - 1; q.invL = (float)(1.0 / L);
    hipLaunchKernelGGL(clf::clf_softmax_kernel, dim3(cdiv(M, 4)), dim3(256), 0, c->s, q);
    CHECK_LAUNCH();
    return 0;
}

// Backward through layer l with the pre-activation delta d of its output over M rows, the
// one-head B_DACT case of core_bwd_layer: the data gradient (d W^T) * f'(in) under the arena th
// into din (nullptr: the first layer, none), then the layer's update with the prior's 1 / s2 (0
// without a prior), masked on a dropout context.
int clf_bwd_layer(vaeb_clf* c, const float* th, const AeLayer& l, float* d, const AeRows& in, int M, float* din) {
    return core_bwd_layer<ae::PAeBwd>(c, th, &l, &d, 1, in, M, ae::B_DACT, din, c->c.prior ? 1.0f / c->c.s2 : 0.f, c->mask,
                                      [](ae::PAeBwd&) {});
}

// One step on the M resident rows idx (a device list): the log-likelihood sum -> outs[slot].
int clf_step(vaeb_clf* c, const int* idx, int M, int slot) {
    const int nh = c->c.n_hidden;
    const float* th = c->theta;
    if (clf_dropout(c)) {
        if (int rc = clf_mask(c, c->step, 0u, c->thm, c->mask)) return rc;
        th = c->thm;
    }
    const AeRows x{c->x, (int)c->nrows, idx};
    if (int rc = clf_forward(c, th, x, M)) return rc;
    if (int rc = clf_softmax(c, M, AeRows{c->y, (int)c->nrows, idx}, c->Pr, c->dA)) return rc;
    hipLaunchKernelGGL(ae::ae_loglik_kernel, dim3(1), dim3(256), 0, c->s, c->rowval, (int64_t)M, 1, c->outs, slot);
    CHECK_LAUNCH();
    if (int rc = clf_bwd_layer(c, th, c->out, c->dA, AeRows{c->H[nh], M, nullptr}, M, c->dH[nh])) return rc;
    for (int i = nh - 1; i > 0; --i)
        if (int rc = clf_bwd_layer(c, th, c->hid[i], c->dH[i + 1], AeRows{c->H[i], M, nullptr}, M, c->dH[i])) return rc;
    if (int rc = clf_bwd_layer(c, th, c->hid[0], c->dH[1], x, M, nullptr)) return rc;
    ++c->step;    // on every context: a schedule means the same with and without dropout
    ++c->opt_t;
    return 0;
}

// The n host rows of x [n x Din] (and of y [n x Dout] when set) in chunks through xin (yin).
template <class Body>
int clf_chunks(vaeb_clf* c, const float* x, const float* y, int64_t n, Body body) {
    return core_chunks(c, n, x, c->c.Din, c->xin, y, c->c.Dout, c->yin, body);
}

// P of the chunk in xin: theta as it is (draws == 0, into Pr) or the mean over the evaluation
// draws 0..draws-1 (into Pacc).  *P: where it is.
int clf_probs(vaeb_clf* c, int rows, int draws, const float** P) {
    const AeRows x{c->xin, rows, nullptr};
    if (draws == 0) {
        *P = c->Pr;
        if (int rc = clf_forward(c, c->theta, x, rows)) return rc;
        return clf_softmax(c, rows, AeRows{}, c->Pr, nullptr);
    }
    *P = c->Pacc;
    for (int l = 0; l < draws; ++l) {
        const float* th = nullptr;
        if (int rc = clf_eval_weights(c, l, &th)) return rc;
        if (int rc = clf_forward(c, th, x, rows)) return rc;
        if (int rc = clf_softmax(c, rows, AeRows{}, nullptr, nullptr, c->Pacc, l, draws)) return rc;
    }
    return 0;
}

int clf_check_draws(const vaeb_clf* c, int64_t draws) {
    if (draws < 0 || draws > (1 << 20)) return fail(VAEB_ERR_ARG, "draws = %lld: 0 to 2^20", (long long)draws);
    if (draws >= 1 && !clf_dropout(c))
        return fail(VAEB_ERR_ARG, "draws = %lld on a context without dropout (draws = 0 uses theta)", (long long)draws);
    return 0;
}

}  // namespace

extern "C" {

int vaeb_clf_create(const vaeb_clf_config* cfg, vaeb_clf** out) {
    if (!cfg || !out) return fail(VAEB_ERR_ARG, "null argument");
    const vaeb_clf_config& g = *cfg;
    if (g.Din <= 0 || g.max_batch <= 0) return fail(VAEB_ERR_ARG, "Din and max_batch must be > 0");
    if (g.n_hidden < 1 || g.n_hidden > VAEB_AE_MAX_LAYERS)
        return fail(VAEB_ERR_ARG, "n_hidden = %d: 1 to %d hidden layers", g.n_hidden, VAEB_AE_MAX_LAYERS);
    for (int i = 0; i < g.n_hidden; ++i) if (g.Dh[i] <= 0) return fail(VAEB_ERR_ARG, "Dh[%d] <= 0", i);
    if (g.Dout < 2) return fail(VAEB_ERR_ARG, "Dout = %d: a softmax needs at least 2 classes", g.Dout);
    if (g.act < 0 || g.act > 2) return fail(VAEB_ERR_ARG, "bad activation");
    if (g.loss != VAEB_CLF_BERNOULLI && g.loss != VAEB_CLF_CATEGORICAL)
        return fail(VAEB_ERR_ARG, "loss must be VAEB_CLF_BERNOULLI | _CATEGORICAL (got %d)", g.loss);
    if (g.prior != 0 && g.prior != 1) return fail(VAEB_ERR_ARG, "prior must be 0 (none) or 1 (N(0, s2)) (got %d)", g.prior);
    if (g.prior == 1 && (!(g.s2 > 0.f) || !std::isfinite(g.s2))) return fail(VAEB_ERR_ARG, "prior 1 needs a finite s2 > 0");
    if (!(g.eta > 0.f) || !std::isfinite(g.eta)) return fail(VAEB_ERR_ARG, "eta must be finite and > 0");
    if (g.dropout != 0 && g.dropout != 1) return fail(VAEB_ERR_ARG, "dropout must be 0 or 1 (got %d)", g.dropout);
    if (g.dropout == 1 && (!(g.keep > 0.f) || !(g.keep <= 1.f)))   // NaN fails both
        return fail(VAEB_ERR_ARG, "dropout needs keep in (0, 1] (got %g)", (double)g.keep);
    auto* c = new vaeb_clf();
    c->c = g;
    c->T = g.dropout ? (uint64_t)std::floor((double)g.keep * 4294967296.0) : 0;
    for (int i = 0; i < g.n_hidden; ++i) { c->hid[i].K = i ? g.Dh[i - 1] : g.Din; c->hid[i].N = g.Dh[i]; }
    c->out.K = g.Dh[g.n_hidden - 1]; c->out.N = g.Dout;
    // theta order (mlp.py:113): the hidden W's, the hidden b's, Wout, bout
    core_place(&c->P, c->hid, g.n_hidden);
    core_place(&c->P, &c->out, 1);
    if (c->P >= (1ll << 31)) {   // the tile kernels' 32-bit byte offsets need less anyway
        const long long P = c->P;
        delete c;
        return fail(VAEB_ERR_ARG, "%lld parameters: the arena holds fewer than 2^31", P);
    }
    int rc = core_open(c, g.device, g.eta, g.act, g.max_batch);
    if (rc) { delete c; return rc; }
    const int64_t B = g.max_batch;
    if (g.dropout) {
        rc = rc ? rc : c->mem.alloc(&c->thm, c->P);
        rc = rc ? rc : c->mem.alloc(&c->mask, c->P);
        rc = rc ? rc : c->mem.alloc(&c->Pacc, B * g.Dout);
    }
    for (int i = 1; i <= g.n_hidden; ++i) {
        rc = rc ? rc : c->mem.alloc(&c->H[i], B * g.Dh[i - 1]);
        rc = rc ? rc : c->mem.alloc(&c->dH[i], B * g.Dh[i - 1]);
    }
    for (float** p : {&c->A, &c->Pr, &c->dA, &c->yin}) rc = rc ? rc : c->mem.alloc(p, B * g.Dout);
    rc = rc ? rc : c->mem.alloc(&c->xin, B * g.Din);
    rc = rc ? rc : c->mem.alloc(&c->rowval, B);
    rc = rc ? rc : c->mem.alloc(&c->hit, B);
    rc = rc ? rc : c->mem.alloc(&c->count, 1);
    rc = rc ? rc : c->mem.alloc(&c->esum, 1);
    if ((rc = core_ready(c, rc))) { delete c; return rc; }
    *out = c;
    return 0;
}

int vaeb_clf_destroy(vaeb_clf* c) {
    if (c) core_close(c);
    delete c;
    return 0;
}

int vaeb_clf_num_params(const vaeb_clf* c, int64_t* n) { return core_num_params(c, n); }

int vaeb_clf_set_data(vaeb_clf* c, const float* x, const float* y, int64_t n_rows) {
    if (!c || !x || !y || n_rows <= 0 || n_rows >= (1ll << 31)) return fail(VAEB_ERR_ARG, "bad data arguments");
    HIP_TRY(hipStreamSynchronize(c->s));
    if (int rc = c->mem.replace(&c->x, n_rows * c->c.Din)) return rc;
    if (int rc = c->mem.replace(&c->y, n_rows * c->c.Dout)) return rc;
    HIP_TRY(hipMemcpy(c->x, x, sizeof(float) * (size_t)n_rows * c->c.Din, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->y, y, sizeof(float) * (size_t)n_rows * c->c.Dout, hipMemcpyHostToDevice));
    c->nrows = n_rows;
    return 0;
}

int vaeb_clf_set_params(vaeb_clf* c, const float* f, int64_t n) { return core_xfer(c, c ? c->theta : nullptr, f, nullptr, n); }
int vaeb_clf_get_params(vaeb_clf* c, float* f, int64_t n) { return core_xfer(c, c ? c->theta : nullptr, nullptr, f, n); }

// The update rule and its state: the core's bodies, as vaeb_ae's.
int vaeb_clf_set_optimizer(vaeb_clf* c, const vaeb_ae_optimizer* o) { return core_set_optimizer(c, o); }
int vaeb_clf_get_optimizer(vaeb_clf* c, vaeb_ae_optimizer* o) { return core_get_optimizer(c, o); }
int vaeb_clf_set_opt_state(vaeb_clf* c, int32_t slot, const float* f, int64_t n) { return core_opt_state(c, slot, f, nullptr, n); }
int vaeb_clf_get_opt_state(vaeb_clf* c, int32_t slot, float* f, int64_t n) { return core_opt_state(c, slot, nullptr, f, n); }
int vaeb_clf_set_opt_step(vaeb_clf* c, int64_t t) { return core_set_opt_step(c, t); }
int vaeb_clf_get_opt_step(vaeb_clf* c, int64_t* t) { return core_get_opt_step(c, t); }

int vaeb_clf_set_seed(vaeb_clf* c, uint64_t seed) {
    if (!c) return fail(VAEB_ERR_ARG, "null argument");
    c->seed = seed;
    return 0;
}

int vaeb_clf_set_step(vaeb_clf* c, int64_t step) {
    if (!c) return fail(VAEB_ERR_ARG, "null argument");
    if (step < 0) return fail(VAEB_ERR_ARG, "step %lld < 0", (long long)step);
    c->step = step;
    return 0;
}

int vaeb_clf_get_step(vaeb_clf* c, int64_t* step) {
    if (!c || !step) return fail(VAEB_ERR_ARG, "null argument");
    *step = c->step;
    return 0;
}

int vaeb_clf_train_many(vaeb_clf* c, const int32_t* idx, int32_t n, int32_t batch, float* out) {
    if (!c) return fail(VAEB_ERR_ARG, "bad arguments");
    return core_train_many(c, c->x, c->nrows, "vaeb_clf_set_data", idx, n, batch, out, [] { return 0; },
                           [c](const int* rows, int m, int slot, int64_t, int64_t) { return clf_step(c, rows, m, slot); });
}

int vaeb_clf_train(vaeb_clf* c, const int32_t* idx, int32_t n, float* out) {
    if (!c || !idx || !out || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (n > c->c.max_batch) return fail(VAEB_ERR_ARG, "n %d > max_batch %d", n, c->c.max_batch);
    return vaeb_clf_train_many(c, idx, n, n, out);
}

int vaeb_clf_predict(vaeb_clf* c, const float* x, int64_t n, int32_t draws, float* out) {
    if (!c || !x || !out || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (int rc = clf_check_draws(c, draws)) return rc;
    const int Dout = c->c.Dout;
    return clf_chunks(c, x, nullptr, n, [&](int64_t r0, int rows) {
        const float* P = nullptr;
        if (int rc = clf_probs(c, rows, draws, &P)) return rc;
        HIP_TRY(hipMemcpyAsync(out + r0 * Dout, P, sizeof(float) * (size_t)rows * Dout, hipMemcpyDeviceToHost, c->s));
        HIP_TRY(hipStreamSynchronize(c->s));
        return 0;
    });
}

int vaeb_clf_loglik(vaeb_clf* c, const float* x, const float* y, int64_t n, int32_t draw, double* out_sum) {
    if (!c || !x || !y || !out_sum || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (draw < -1 || draw >= (1 << 20)) return fail(VAEB_ERR_ARG, "draw = %d: -1 (theta) or 0 to 2^20 - 1", draw);
    if (draw >= 0 && !clf_dropout(c)) return fail(VAEB_ERR_ARG, "draw = %d on a context without dropout (-1 uses theta)", draw);
    double total = 0.0;
    const int rc = clf_chunks(c, x, y, n, [&](int64_t, int rows) {
        const float* th = nullptr;
        if (int rc = clf_eval_weights(c, draw, &th)) return rc;
        if (int rc = clf_forward(c, th, AeRows{c->xin, rows, nullptr}, rows)) return rc;
        if (int rc = clf_softmax(c, rows, AeRows{c->yin, rows, nullptr}, nullptr, nullptr)) return rc;
        return core_sum_to_host(c, c->rowval, rows, &total);
    });
    if (rc) return rc;
    *out_sum = total;
    return 0;
}

int vaeb_clf_accuracy(vaeb_clf* c, const float* x, const float* y, int64_t n, int32_t draws, int64_t* correct) {
    if (!c || !x || !y || !correct || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (int rc = clf_check_draws(c, draws)) return rc;
    HIP_TRY(hipMemsetAsync(c->count, 0, sizeof(long long), c->s));
    const int rc = clf_chunks(c, x, y, n, [&](int64_t, int rows) {
        const float* P = nullptr;
        if (int rc = clf_probs(c, rows, draws, &P)) return rc;
        hipLaunchKernelGGL(clf::clf_hit_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, c->s, P, (const float*)c->yin, rows,
                           c->c.Dout, c->hit);
        CHECK_LAUNCH();
        hipLaunchKernelGGL(clf::clf_count_kernel, dim3(1), dim3(256), 0, c->s, (const int*)c->hit, rows, c->count);
        CHECK_LAUNCH();
        HIP_TRY(hipStreamSynchronize(c->s));   // xin / yin are free for the next chunk's upload
        return 0;
    });
    if (rc) return rc;
    long long got = 0;
    HIP_TRY(hipMemcpyAsync(&got, c->count, sizeof(long long), hipMemcpyDeviceToHost, c->s));
    HIP_TRY(hipStreamSynchronize(c->s));
    *correct = got;
    return 0;
}

int vaeb_clf_draw_mask(vaeb_clf* c, int64_t step, int32_t draw, uint8_t* out) {
    if (!c || !out) return fail(VAEB_ERR_ARG, "null argument");
    if (!clf_dropout(c)) return fail(VAEB_ERR_ARG, "vaeb_clf_draw_mask needs a dropout context");
    if (step < 0 || draw < -1 || draw >= (1 << 20)) return fail(VAEB_ERR_ARG, "bad step %lld or draw %d", (long long)step, draw);
    if (int rc = clf_mask(c, step, draw < 0 ? 0u : 1u | ((uint32_t)(draw + 1) << 1), nullptr, c->mask)) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->mask, (size_t)c->P, hipMemcpyDeviceToHost, c->s));
    HIP_TRY(hipStreamSynchronize(c->s));
    return 0;
}

}  // extern "C"
