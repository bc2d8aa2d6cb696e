// engine_f32.inc -- the host side of the fp32 step engine (the headline path: MNIST 784-500-20,
// batch 100): launch arguments, the launch helpers that map run-time shapes onto the kernels'
// compile-time parameters, the forward and the training step, and the fp32 evaluation chunks.
// Included once by vaeb_hip.hip inside its anonymous namespace, ahead of the 16-bit engine
// (which shares cdiv, make_opt and the profiling brackets).

// f(std::integral_constant<T, V>{}) for the V of the list Vs that equals the run-time v: the one
// way a run-time value becomes a kernel's template argument here.  False when no V matches.
template <auto... Vs, class T, class F>
bool dispatch(T v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<decltype(Vs), Vs>{}), true) : false) || ...);
}

uint64_t* next_dbg(vaeb_ctx* c) { return c->dbg ? c->dbg + (size_t)(c->dbg_slot++) * kDbgWG * 8 : nullptr; }

StepArgs make_args(vaeb_ctx* c, int par, int Mb, int mode, const float* xbase, bool train) {
    StepArgs a{};
    const vaeb_config& g = c->c;
    a.D = g.D; a.H = g.H; a.Z = g.Z; a.L = g.L;
    a.Mb = Mb; a.Mbp = r16(Mb); a.Me = g.L * a.Mbp;
    a.dec = g.decoder; a.est = g.estimator == VAEB_EST_FVS ? VAEB_EST_LB : g.estimator; a.mode = mode;
    a.sc = (g.objective == VAEB_OBJ_MEAN_MAP) ? 1.0f / (float)g.B_global : 1.0f;
    const float* t = c->theta2[par];
    const ArenaSlots& sl = c->sl;
    auto at = [&](int slot) { return slot >= 0 ? t + c->off[slot] : nullptr; };
    a.W3 = at(sl.W3); a.W4 = at(sl.W4); a.W5 = at(sl.W5); a.W1 = at(sl.W1); a.W2 = at(sl.W2); a.W6 = at(sl.W6);
    a.b3 = at(sl.b3); a.b4 = at(sl.b4); a.b5 = at(sl.b5); a.b1 = at(sl.b1); a.b2 = at(sl.b2); a.b6 = at(sl.b6);
    a.xbase = xbase;
    if (train) {
        // this rank's rows of global minibatch b start at row b * B_global + row_offset
        a.xbase = xbase + (int64_t)g.row_offset * g.D;
        a.order = c->ictl + kCtlOrder;
        a.cursor = c->ictl;
        a.cur_batch = c->ictl + 1;
        a.batch_stride = (int64_t)g.B_global * g.D;
        a.row_base_mul = g.B_global;
        a.row_base_add = g.row_offset;
        a.domain = 0;
    } else {   // rows at xbase: no order, no cursor, no batch stride
        a.cur_batch = c->ictl + 1;
        a.domain = 1;
    }
    a.eps_mode = (mode == MODE_RECON) ? 2 : (c->eps_mode == VAEB_EPS_HOST ? 1 : 0);
    a.seed = c->seed;
    a.step = c->step;
    a.eps_in = c->eps_in;
    a.eps_in_ld = c->eps_rows;
    a.h = c->h; a.mu = c->mu; a.lv = c->lv; a.eps = c->eps; a.z = c->z; a.hd = c->hd; a.y = c->y;
    a.dA2 = c->dA2; a.dA6 = c->dA6; a.dA1 = c->dA1; a.dZ = c->dZ; a.dMuLv = c->dMuLv; a.dA3 = c->dA3;
    a.kl_part = c->kl_part; a.la_part = c->kl_part; a.lp_part = c->lp_part;
    a.nctZ = cdiv(g.Z, 16);
    a.nctD = cdiv(g.D, 16);
    a.slab_ml = c->slab_ml; a.slab_dz = c->slab_dz; a.cnt_ml = c->cnt_ml; a.cnt_dz = c->cnt_dz;
    a.acc_ml = c->acc_ml; a.acc_dz = c->acc_dz;
    return a;
}

ElboArgs base_elbo(vaeb_ctx* c, const StepArgs& a) {
    ElboArgs e{};
    e.lp_part = c->lp_part; e.n_lp = (int64_t)a.Me * a.nctD;
    e.kl_part = c->kl_part;
    e.n_kl = (int64_t)(c->c.estimator == VAEB_EST_LA ? a.Me : a.Mbp) * a.nctZ;
    e.L = c->c.L; e.est = c->c.estimator;
    e.data_mul = 1.0;
    e.inv_bglob = 1.0 / (double)c->c.B_global;
    return e;
}

OptArgs make_opt(vaeb_ctx* c, int par, bool update, bool store) {
    OptArgs o{};
    o.theta_in = c->theta2[par];
    o.theta_out = c->theta2[par ^ 1];
    o.acc = c->acc; o.grad = c->grad;
    o.lr = c->c.lr; o.eps = c->c.adagrad_eps;
    const bool mean = c->c.objective == VAEB_OBJ_MEAN_MAP;
    o.prior = mean ? 0.f : 1.f;
    o.decay = mean ? c->c.lr * c->c.adagrad_eps : 0.f;
    o.update = update ? 1 : 0;
    o.store_grad = store ? 1 : 0;
    return o;
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
int latent_tiles(const StepArgs& a) { return a.Z <= 16 ? 1 : 2; }   // NCT: 16-column latent tiles (Z <= 32)
// GCH, the K chunks a wave of the 8-wave main loops keeps in flight: 8 when K > 512 ("deep")
int chunk_group(int K) { return cdiv(cdiv(K, 16), 8) > 4 ? 8 : 4; }

// ------------------------------------------------------------------ forms and plans
bool fused_latent(const vaeb_ctx* c) { return c->c.Z <= 32; }
// Training minibatches with Z <= 32 fold the latent block into the wide phases
// (latent.hpp); validation / reconstruction chunks keep the per-row-block kernels.
bool folded_latent(const vaeb_ctx* c, const StepArgs& a) {
    return fused_latent(c) && a.domain == 0 && a.Mbp <= r16(c->c.B);   // training rows (domain 0)
}

// Weight-gradient tile widths (columns; rows are kWT = 64).  Narrower tiles mean more
// workgroups, each streaming fewer theta / accumulator / panel bytes through its CU: at
// MNIST-20, 64 -> 32 wide took the dW2 launch 11.7 -> 9.5 us and the dW3 | dW45 launch
// 10.9 -> 8.1 us; 16 wide takes the latter to 7.5 us but the dW2 launch (beside 224 dhd
// tiles) back up to 11.1 us.
constexpr int kWTJ_P5 = 32;    // dW2 (| dW6), beside the dhd tiles (64 wide: 40.1 vs 38.8 us per step)
constexpr int kW3TS = 1;       // 16-column groups per tile of the last launch (dW3 | dW45 | dW1; 2: 40.1 vs 38.8)
constexpr int kWTJ_P67 = 16;   // dW1, beside the dz / dh phase
constexpr int kWTJ_W = 16;     // standalone launches: dW3 | dW45 (+ ELBO), non-fused dW1
constexpr int kDzSplit = 8;    // P67 column splits per row block (fused.hpp dz_dh_body)

// The folded latent hand-offs: counted fixed-point atomics (latent.hpp fx_*) or slabs +
// ticket + reducer.  The returning adds to one accumulator serialise at the memory side, so
// the atomic form wins only at a small fan-in (contributors per element): Frey 560-200-2
// (13 column tiles) 38.5 -> 32.2 us per step; MNIST 784-500-20 (32 column tiles) 44.5 ->
// 49.3 us.  Forward fan-in: the H column tiles; backward: H column tiles x L planes.
// (A third form -- the same adds without return + the slab protocol's ticket, the last
// arriver reading each sum with one exchange -- measured slower than both, MNIST 53.6 us,
// Frey 35.0 us, and was removed in round 3.)  VAEB_ATOMIC_HO=0 forces the slabs.
int ho_mode(const vaeb_ctx* c, int fan_in) {
    if (c->atomic_ho == 0) return 0;
    return fan_in <= kFxMaxFanIn ? 1 : 0;   // the count field holds <= 16 contributors (latent.hpp)
}
int ho_ml(const vaeb_ctx* c, int ct) { return ho_mode(c, cdiv(c->c.H, 16 * ct)); }
// backward: 1 atomic, else 2 (deferred to the last launch's reducers, VAEB_BWD_DEFER) or 0
// (ticket).  (Round 5's form 3 -- two dA1 column tiles per 1024-thread dhd workgroup so MNIST's
// fan-in fits the counted atomics -- measured 39.4 vs 34.4 us per step and was removed in round 6.)
int ho_dz(const vaeb_ctx* c) {
    const int m = ho_mode(c, cdiv(c->c.H, 16) * c->c.L);
    return m == 0 && c->bwd_defer ? 2 : m;
}

// The encoder form the folded forward takes for `a` (enqueue_forward): ho (3 slabs summed by
// the decoder, 1 counted atomics, 0 ticket), ct column tiles per workgroup; w16 when that
// form runs on 16-wave workgroups (enc_latent16_kernel), the one that can carry the deferred dW2.
struct EncForm {
    int ho, ct;
    bool red, w16;
};
EncForm enc_form(const vaeb_ctx* c, const StepArgs& a, const FvFold& fvf = FvFold{}) {
    const bool red = (c->enc_red < 0 ? ho_ml(c, 1) == 0 : c->enc_red == 1) && fvf.rows == 0 && cdiv(a.H, 32) <= 32;
    const int ct = (red || fvf.rows > 0) ? 2 : 1;
    // (round 4's HO 4 -- the [mu | lv] partials as exact fixed-point sums read by the decoder,
    // VAEB_ENC_FX -- measured 34.8-35.1 vs 34.4-34.5 us per step and was removed in round 6)
    const int ho = red ? 3 : ho_ml(c, ct);
    return EncForm{ho, ct, red, ho == 3 || (ho == 1 && fvf.rows == 0 && ct == 1)};
}

// The deferred dW2's launch arguments (the previous step's dW2 (| dW6) group; vaeb_ctx::dw2_defer)
struct W2Launch {
    WGradArgs w;
    bool vec;
    const int* pend;
    int width;     // tile columns (w2_plan)
    bool paired;   // two tiles per workgroup, after the encoder rows
};

// The deferred dW2's tiling (latent.hpp enc_latent16_w2_kernel).  One 64 x width tile per
// workgroup, each on a CU of its own beside the encoder's `enc_wgs` workgroups: the narrowest of
// 32, 48 and 64 columns whose tile count fits the CUs left free (narrower tiles stream fewer
// theta / Adagrad / panel bytes through one CU's load path; MNIST 784-500: 17 x 8 = 136 tiles
// of 48 beside 112 encoder workgroups).  Where none fits (or VAEB_DW2_PAIRED=1): 32-wide tiles,
// two per workgroup.  rows = H + 1 (the bias row), cols = D (Gaussian: [W2 | W6] = 2 D).
// wide64: 64 columns are a candidate -- only with 16-byte accesses (the scalar epilogue's
// per-element offsets, theta and Adagrad state of 64 columns do not fit 128 VGPRs).
constexpr int kCUs = 256;
struct W2Plan {
    int width, paired, tiles_i, tiles_j;   // tile (row block i, column block j) = worker i * tiles_j + j
};
W2Plan w2_plan(int rows, int cols, int enc_wgs, bool force_paired, bool wide64) {
    const int ti = cdiv(rows, kWT);
    if (!force_paired)
        for (int w : {32, 48, 64}) {
            if (w == 64 && !wide64) break;
            const int tj = cdiv(cols, w);
            if (ti * tj <= kCUs - enc_wgs) return W2Plan{w, 0, ti, tj};
        }
    return W2Plan{kWTJ_P5, 1, ti, cdiv(cols, kWTJ_P5)};
}

// ------------------------------------------------------------------ weight-gradient groups
WGroup make_group(const vaeb_ctx* c, const float* at, int ld_at, int klim, int at_is_x, int rowsW, const float* b0,
                  int ld0, int N0, const float* b1, int ld1, int N1, int K, int pW0, int pb0, int pW1, int pb1) {
    WGroup G{};
    G.at = at; G.ld_at = ld_at; G.klim_at = klim; G.at_is_x = at_is_x; G.rowsW = rowsW;
    G.b0 = b0; G.ld0 = ld0; G.N0 = N0; G.b1 = b1; G.ld1 = ld1; G.N1 = N1; G.K = K;
    G.offW0 = c->off[pW0]; G.offb0 = c->off[pb0];
    G.offW1 = pW1 >= 0 ? c->off[pW1] : 0; G.offb1 = pb1 >= 0 ? c->off[pb1] : 0;
    return G;
}
// The dW2 (| dW6) weight-gradient group -- [hd | 1]^T [dA2 (| dA6)]
WGroup w2_group(const vaeb_ctx* c, const StepArgs& a) {
    const bool gs = gaussian(c);
    return make_group(c, c->hd, a.H, a.Me, 0, a.H, c->dA2, a.D, a.D, gs ? c->dA6 : nullptr, a.D, gs ? a.D : 0, a.Me,
                      c->sl.W2, c->sl.b2, c->sl.W6, c->sl.b6);
}

// Whether group G's tiles may use 16-byte accesses: panel loads need every panel row aligned
// with widths % 4 == 0 (the activation buffers are hipMalloc'd; X rows are D floats apart),
// (and 16-byte theta / Adagrad-state accesses in the epilogue: arena offsets % 4 == 0).
// (A host-only context's null pointers count as aligned, as its device allocations would be.)
bool group_vec16(const vaeb_ctx* c, const WGroup& G, const float* xbase) {
    return (G.ld_at % 4 == 0) && (G.rowsW % 4 == 0) && aligned16(G.at_is_x ? xbase : G.at) &&
           (G.ld0 % 4 == 0) && (G.N0 % 4 == 0) && aligned16(G.b0) && G.offW0 % 4 == 0 && G.offb0 % 4 == 0 &&
           (G.N1 == 0 || ((G.ld1 % 4 == 0) && (G.N1 % 4 == 0) && aligned16(G.b1) && G.offW1 % 4 == 0 &&
                          G.offb1 % 4 == 0)) &&
           aligned16(c->theta2[0]) && aligned16(c->theta2[1]) && aligned16(c->acc) && aligned16(c->grad);
}

void set_head(WGradArgs& w, int n, int total, bool elbo, const float* xb, const int* cb, int64_t bs) {
    w.ngroups = n; w.total_wgs = total; w.with_elbo = elbo; w.xbase = xb; w.cur_batch = cb; w.batch_stride = bs;
}
void set_head(WGradArgs3& w, int n, int total, bool elbo, const float* xb, const int* cb, int64_t bs) {
    W3Head& h = w.hd;
    h.ngroups = n; h.total_wgs = total; h.with_elbo = elbo; h.xbase = xb; h.cur_batch = cb; h.batch_stride = bs;
    h.gb1 = n > 1 ? w.g[1].wg_begin : total; h.gb2 = n > 2 ? w.g[2].wg_begin : total;
    h.nred = 0; h.red_cnt = nullptr;
}

// Weight-gradient arguments over `n` groups whose tiles start at block `base` of the
// launch (+ the ELBO workgroup when e != nullptr).  *vec: 16-byte panel loads are legal.
template <class WA>
int prep_wgrad(vaeb_ctx* c, const WGroup* groups, int n, const OptArgs& opt, const ElboArgs* e, const StepArgs& a,
               int base, WA& w, bool& vec, int tw, int* vmask = nullptr) {
    w = WA{};
    int begin = base;
    constexpr int kMaxG = (int)(sizeof(w.g) / sizeof(w.g[0]));
    if (n < 1 || n > kMaxG) return fail(VAEB_ERR_ARG, "internal: 1 to %d weight-gradient groups per launch", kMaxG);
    for (int gi = 0; gi < n; ++gi) {
        w.g[gi] = groups[gi];
        WGroup& G = w.g[gi];
        G.tiles_j = cdiv(G.N0 + G.N1, tw);
        G.wg_begin = begin;
        G.wg_end = begin + cdiv(G.rowsW + 1, kWT) * G.tiles_j;
        begin = G.wg_end;
    }
    set_head(w, n, begin, e != nullptr, a.xbase, c->ictl + 1, a.batch_stride);
    w.opt = opt;
    if (e) w.elbo = *e;
    w.P = c->P;
    w.dbg = a.dbg;
    vec = true;
    if (vmask) *vmask = 0;
    for (int gi = 0; gi < n; ++gi) {
        const bool gv = group_vec16(c, w.g[gi], a.xbase);
        vec = vec && gv;
        if (vmask && gv) *vmask |= 1 << gi;
    }
    return 0;
}

// The dW2 (| dW6) group as launch arguments whose tiles start at block `base`, with the
// optimizer `opt`.
int w2_args(vaeb_ctx* c, const StepArgs& a, const OptArgs& opt, int base, WGradArgs& w, bool& vec, int tw = kWTJ_P5) {
    const WGroup g4 = w2_group(c, a);
    return prep_wgrad(c, &g4, 1, opt, nullptr, a, base, w, vec, tw);
}
// The deferred dW2's tiling for the training step on `a` (its encoder grid: enqueue_forward).
W2Plan w2_plan_for(const vaeb_ctx* c, const StepArgs& a) {
    const int enc_wgs = (a.Mbp / 16) * cdiv(a.H, 16 * enc_form(c, a).ct);
    return w2_plan(a.H + 1, (gaussian(c) ? 2 : 1) * a.D, enc_wgs, c->dw2_paired, group_vec16(c, w2_group(c, a), a.xbase));
}

// Whether the step on `a` defers its dW2 into the next step's encoder launch (vaeb_ctx::dw2_defer).
// Only where the dhd launch hands its latent backward to the last launch (ho_dz 2): there the
// dW2 tiles bound the dhd launch.  With the counted atomic backward (small fan-in: Frey) the dhd
// launch is bound by that hand-off and hides dW2, while the encoder would pay for it: Frey
// 29.78 / 29.87 µs in-step vs 31.54 / 31.55 deferred.
bool dw2_deferrable(const vaeb_ctx* c) {
    const int est = c->c.estimator;
    StepArgs a{};
    a.H = c->c.H;   // (all enc_form reads of the training step's arguments)
    return c->dw2_defer && c->c.dtype == VAEB_DTYPE_F32 && c->comm == nullptr && est != VAEB_EST_FV && est != VAEB_EST_FVS &&
           fused_latent(c) && c->fold_bwd && enc_form(c, a).w16;
}
bool dw2_deferred(const vaeb_ctx* c, const StepArgs& a) {
    const int hd = ho_dz(c);
    return dw2_deferrable(c) && hd == 2 && folded_latent(c, a);
}

// ------------------------------------------------------------------ launch helpers
template <int WM, int WN, int KS, int NB, int GCH, class P>
void launch_tile(hipStream_t s, const P& p) {
    dim3 grid(cdiv(p.M, 16 * WM), cdiv(p.N, 16 * WN));
    hipLaunchKernelGGL((tile_kernel<WM, WN, KS, NB, GCH, P>), grid, dim3(64 * WM * WN * KS), 0, s, p);
}

// Big-K phases: 8 waves split K; a wave's chunks go in flight together (GCH per trip).
template <int NB, class P>
void launch_bigk(hipStream_t s, const P& p) {
    dispatch<4, 8>(chunk_group(p.K), [&](auto GCH) { launch_tile<1, 1, 8, NB, decltype(GCH)::value>(s, p); });
}
// P4 of the per-row-block forward: Bernoulli means, or Gaussian means and log-variances
void launch_decout(const vaeb_ctx* c, hipStream_t s, const StepArgs& a) {
    if (gaussian(c)) launch_bigk<2>(s, PDecOut{a, nullptr, a.Me, a.D, a.H});
    else launch_bigk<1>(s, PDecOut{a, nullptr, a.Me, a.D, a.H});
}
void launch_heads_dechid(hipStream_t s, const StepArgs& a) {
    dispatch<1, 2>(latent_tiles(a), [&](auto NCT) {
        hipLaunchKernelGGL(heads_dechid_kernel<decltype(NCT)::value>, dim3(a.Mbp / 16), dim3(512), 0, s, a);
    });
}

// decout_z_kernel / decout_z2_kernel at compile-time NB (output planes), ZM (latent quads held
// per thread), V1 (16-byte W1 / b1 loads) and AT (the encoder's hand-off form)
template <int NB, int AT>
void launch_decout_z(hipStream_t s, dim3 grid, const StepArgs& a, int ct = 1) {
    const int q = (a.Z + 3) / 4, zm = q <= 2 ? q : q <= 4 ? 4 : q == 5 ? 5 : 8;
    dispatch<false, true>((a.H & 3) == 0 && aligned16(a.W1) && aligned16(a.b1), [&](auto V1) {
        dispatch<1, 2, 4, 5, 8>(zm, [&](auto ZM) {
            constexpr bool v1 = decltype(V1)::value;
            constexpr int z = decltype(ZM)::value;
            if constexpr (NB == 1) {
                if (ct == 2) {   // two column tiles per workgroup
                    hipLaunchKernelGGL((decout_z2_kernel<z, v1, AT>), grid, dim3(512), 0, s, a);
                    return;
                }
            }
            hipLaunchKernelGGL((decout_z_kernel<NB, z, v1, AT>), grid, dim3(512), 0, s, a);
        });
    });
}

// dhd_dz_wgrad_kernel at compile-time NCT (latent col tiles), GCH, load width, AT
template <int TS, int HO>
void launch_dhd_dz(hipStream_t s, dim3 grid, const PDhdT<true>& p5, const PDhdT<false>& p5s, const WGradArgs& w,
                   int ntile, int gx, bool vec, bool deep, DhdAux pend) {
    dispatch<1, 2>(latent_tiles(p5.a), [&](auto NCT) {
        dispatch<4, 8>(deep ? 8 : 4, [&](auto GCH) {
            constexpr int nct = decltype(NCT)::value, gch = decltype(GCH)::value;
            if (vec) hipLaunchKernelGGL((dhd_dz_wgrad_kernel<nct, gch, true, TS, HO>), grid, dim3(512), 0, s, p5, w, ntile, gx, pend);
            else hipLaunchKernelGGL((dhd_dz_wgrad_kernel<nct, gch, false, TS, HO>), grid, dim3(512), 0, s, p5s, w, ntile, gx, pend);
        });
    });
}

// enc_latent_kernel / enc_latent_fv_kernel at compile-time NCT (latent col tiles), GCH
// (main-loop chunk group), AT (atomic hand-off)
template <int HO, int CT>
void launch_enc_latent_ct(hipStream_t s, dim3 g1, const StepArgs& a, const FvFold& fvf, bool deep) {
    dispatch<1, 2>(latent_tiles(a), [&](auto NCT) {
        dispatch<4, 8>(deep ? 8 : 4, [&](auto GCH) {
            constexpr int nct = decltype(NCT)::value, gch = decltype(GCH)::value;
            if (fvf.rows > 0) hipLaunchKernelGGL((enc_latent_fv_kernel<nct, gch, HO, CT>), g1, dim3(512), 0, s, a, fvf);
            else hipLaunchKernelGGL((enc_latent_kernel<nct, gch, HO, CT>), g1, dim3(512), 0, s, a);
        });
    });
}
template <int HO, int CT>
void launch_enc16(hipStream_t s, dim3 g1, const StepArgs& a) {
    dispatch<1, 2>(latent_tiles(a), [&](auto NCT) {
        hipLaunchKernelGGL((enc_latent16_kernel<decltype(NCT)::value, 4, HO, CT>), g1, dim3(1024), 0, s, a);
    });
}
// The 16-wave encoder with the deferred dW2 workers (w2: the previous step's dW2 group) in
// ceil(workgroups / (Mbp / 16)) extra grid rows: ahead of the encoder rows with one tile per
// workgroup, behind them in the paired form (and in the timeline build, whose stamps index the
// encoder's workgroups from 0).
template <int HO, int CT, int TS, int NW>
void launch_enc16_w2_ts(hipStream_t s, dim3 g1, const StepArgs& a, const W2Launch& w2) {
    const int rows_enc = (int)g1.y, rows_w2 = cdiv(cdiv(w2.w.total_wgs, NW), (int)g1.x);
#ifdef VAEB_TIMELINE
    const bool first = false;
#else
    const bool first = NW == 1;
#endif
    const int y_enc = first ? rows_w2 : 0, y_w2 = first ? 0 : rows_enc;
    const dim3 g(g1.x, rows_enc + rows_w2);
    dispatch<1, 2>(latent_tiles(a), [&](auto NCT) {
        dispatch<false, true>(TS == 4 || w2.vec, [&](auto VEC) {
            constexpr bool vec = decltype(VEC)::value;
            if constexpr (vec || TS < 4)   // 64 columns: planned only with 16-byte accesses (w2_plan)
                hipLaunchKernelGGL((enc_latent16_w2_kernel<decltype(NCT)::value, 4, HO, CT, vec, TS, NW>), g, dim3(1024),
                                   0, s, a, w2.w, w2.pend, y_enc, y_w2, rows_w2);
        });
    });
}
template <int HO, int CT>
bool launch_enc16_w2(hipStream_t s, dim3 g1, const StepArgs& a, const W2Launch& w2) {   // false: no such width
    if (w2.paired) return launch_enc16_w2_ts<HO, CT, kWTJ_P5 / 16, 2>(s, g1, a, w2), true;
    return dispatch<2, 3, 4>(w2.width / 16, [&](auto TS) { launch_enc16_w2_ts<HO, CT, decltype(TS)::value, 1>(s, g1, a, w2); });
}

// The slab-only encoder (HO 3: partials summed by the decoder launch, CT = 2, no FV) and the
// atomic hand-off encoder (HO 1, one column tile, no FV) run on 1024-thread workgroups, 16
// waves splitting K (twice the loads in flight per CU): MNIST 38.82 -> 37.87 us/step, Frey
// 29.19 -> 29.01 in round 3's alternating runs (the 512-thread forms' switch, VAEB_ENC16, was
// removed in round 6).  The ticketed reducer (HO 0) and the FV-stream encoder keep 512 threads.
template <int HO>
bool launch_enc_latent(hipStream_t s, dim3 g1, const StepArgs& a, const FvFold& fvf, bool deep, int ct,
                       const W2Launch* w2 = nullptr) {
    if constexpr (HO == 3) {
        if (w2) return launch_enc16_w2<HO, 2>(s, g1, a, *w2);
        return launch_enc16<HO, 2>(s, g1, a), true;
    }
    if constexpr (HO == 1) {
        if (fvf.rows == 0 && ct == 1) {   // the atomic hand-off on 16 waves
            if (w2) return launch_enc16_w2<1, 1>(s, g1, a, *w2);
            return launch_enc16<1, 1>(s, g1, a), true;
        }
    }
    return dispatch<1, 2>(ct, [&](auto CT) { launch_enc_latent_ct<HO, decltype(CT)::value>(s, g1, a, fvf, deep); });
}

// A standalone weight-gradient launch (256-thread blocks).  da3: group 0 (dW3) forms its
// dA3 panel from [dMu | dLv] in the workgroup (the folded latent backward).
int launch_wgrad(vaeb_ctx* c, hipStream_t s, const WGroup* groups, int n, const OptArgs& opt, const ElboArgs* e,
                 const StepArgs& a, const Da3Src* da3 = nullptr) {
    bool vec;
    if (da3) {
        if (n != 3) return fail(VAEB_ERR_ARG, "internal: the dA3-forming launch takes three groups");
        WGradArgs3 w;
        // 16-column tiles (32-wide: MNIST 46.3 vs 44.7 us, Frey 41.5 vs 38.4 in round 2;
        // -DVAEB_W3_TS=2 builds them for A/B)
        int vm = 0;   // 16-byte panel loads per group (Frey: dW3 yes, dW4 | dW5 and dW1 not)
        if (int rc = prep_wgrad(c, groups, n, opt, e, a, 0, w, vec, 16 * kW3TS, &vm)) return rc;
        w.da3 = *da3;
        const int nred = da3->red.nred;
        w.hd.nred = nred;
        w.hd.red_cnt = da3->red.cnt;
        const dim3 grid(w.hd.total_wgs + (e ? 1 : 0) + nred);
        // DEFER: reducers in this launch, or [dMu | dLv] handed in by the dhd launch
        dispatch<false, true>(nred > 0, [&](auto DF) {
            // (the kernel exists for the masks that hold group 0, dW3; any other runs all scalar)
            dispatch<0, 1, 3, 5, 7>((vm & 1) ? vm : 0, [&](auto VM) {
                hipLaunchKernelGGL((wgrad3_kernel<decltype(VM)::value, kW3TS, decltype(DF)::value>), grid, dim3(256), 0, s, w);
            });
        });
    } else {
        WGradArgs w;
        if (int rc = prep_wgrad(c, groups, n, opt, e, a, 0, w, vec, kWTJ_W)) return rc;
        const dim3 grid(w.total_wgs + (e ? 1 : 0));
        dispatch<false, true>(vec, [&](auto VEC) {
            hipLaunchKernelGGL((wgrad_kernel<decltype(VEC)::value, kWTJ_W / 16>), grid, dim3(256), 0, s, w);
        });
    }
    CHECK_LAUNCH();
    return 0;
}

// Run the pending step's dW2 (| dW6) + Adagrad now (their own launch; the device flag makes it
// a no-op when a later step's encoder already ran them): every host read or write of the
// parameters, the Adagrad state or the gradient, every evaluation, comes after it.
int w2_flush(vaeb_ctx* c) {
    if (!c || !c->w2_dirty) return 0;
    c->w2_dirty = false;
    const int par = c->par;   // the arena the next step reads: the pending dW2 writes W2' there
    StepArgs a = make_args(c, par, c->c.B, MODE_TRAIN, c->data, true);
    WGradArgs w;
    bool vec;
    const int tw = w2_plan_for(c, a).width;   // the width of the deferred launch this one replaces
    if (int rc = w2_args(c, a, make_opt(c, par ^ 1, true, c->c.keep_grads != 0), 0, w, vec, tw)) return rc;
    w.dbg = nullptr;
    if (tw == 64 && !vec) return fail(VAEB_ERR_ARG, "internal: 64-wide dW2 tiles need 16-byte accesses");
    if (!dispatch<2, 3, 4>(tw / 16, [&](auto TS) {
        constexpr int ts = decltype(TS)::value;
        if (vec) hipLaunchKernelGGL((w2_flush_kernel<true, ts>), dim3(w.total_wgs), dim3(512), 0, c->s, w, c->w2pend);
        else if constexpr (ts < 4) hipLaunchKernelGGL((w2_flush_kernel<false, ts>), dim3(w.total_wgs), dim3(512), 0, c->s, w, c->w2pend);
    })) return fail(VAEB_ERR_ARG, "internal: no dW2 flush kernel for %d-wide tiles", tw);
    CHECK_LAUNCH();
    HIP_TRY(hipMemsetAsync(c->w2pend, 0, sizeof(int), c->s));
    return 0;
}

// ------------------------------------------------------------------ the forward
// Forward phases P1..P4 for any mode.
int enqueue_forward(vaeb_ctx* c, const StepArgs& a0, Prof& pr, const FvFold& fvf = FvFold{},
                    const W2Launch* w2 = nullptr) {
    hipStream_t s = c->s;
    StepArgs a = a0;
    a.dbg = next_dbg(c);
    if (folded_latent(c, a)) {
        // auto: two column tiles per workgroup when the literal-FV stream shares the launch
        // (FV 27.75 -> 27.4 us: fewer encoder tiles beside the stream blocks), else one
        // (MNIST 44.6 either way, Frey 32.2 vs 34.0 us)
        // VAEB_ENC_RED=1: no hand-off in the encoder launch at all -- its CT = 2 tiles store
        // partial [mu | lv] slabs and end; every decoder workgroup sums its row block's
        // ceil(H / 32) slabs (decout_z_kernel<.., ZM = 2>)
        // auto: where the slab + ticket form would be chosen (fan-in > 16; MNIST 784-500-20
        // 43.8 -> 42.5 us); at a small fan-in the counted atomics stay (Frey 30.8 vs 32.7 us)
        const EncForm f = enc_form(c, a, fvf);
        const dim3 g1(a.Mbp / 16, cdiv(a.H, 16 * f.ct) + fvf.rows);
        const bool deep = chunk_group(a.D) == 8;
        const int at = f.red ? 2 : (f.ho == 1 ? 1 : 0);
        pr.mark(w2 ? K_P1_ENC_LATENT_W2 : K_P1_ENC_LATENT);
        bool ok = true;   // false: a value outside a dispatch list (no launch was made)
        REP(pr) ok = dispatch<0, 1, 3>(f.ho, [&](auto HO) { ok = ok && launch_enc_latent<decltype(HO)::value>(s, g1, a, fvf, deep, f.ct, w2); }) && ok;
        if (!ok) return fail(VAEB_ERR_ARG, "internal: no encoder launch for hand-off %d, %d column tiles, dW2 width %d", f.ho, f.ct, w2 ? w2->width : 0);
        CHECK_LAUNCH();
        if (int rc = order_hook(c)) return rc;
        a.dbg = next_dbg(c);
        // Bernoulli: two 16-column tiles per workgroup (decout_z2_kernel; one tile: 42.0 vs
        // 39.4 us per step in round 3, its switch VAEB_DECOUT_CT removed in round 6)
        const int dct = gaussian(c) ? 1 : 2;
        const dim3 g4(a.Me / 16, cdiv(a.D, 16 * dct));
        pr.mark(K_P4_DECOUT_Z);
        REP(pr) dispatch<0, 1, 2>(at, [&](auto AT) {
            if (gaussian(c)) launch_decout_z<2, decltype(AT)::value>(s, g4, a);
            else launch_decout_z<1, decltype(AT)::value>(s, g4, a, dct);
        });
        CHECK_LAUNCH();
        return 0;
    }
    pr.mark(K_P1_ENC);
    REP(pr) launch_bigk<1>(s, PEnc{a, nullptr, a.Mbp, a.H, a.D});
    CHECK_LAUNCH();
    a.dbg = next_dbg(c);
    if (fused_latent(c)) {
        pr.mark(K_P23_HEADS_DECHID);
        REP(pr) launch_heads_dechid(s, a);
        CHECK_LAUNCH();
    } else {
        pr.mark(K_P2_HEADS);
        REP(pr) launch_tile<1, 1, 4, 2, 8>(s, PHeads{a, a.Mbp, a.Z, a.H});
        CHECK_LAUNCH();
        pr.mark(K_P3_DECHID);
        REP(pr) launch_tile<1, 4, 1, 1, 8>(s, PDecHid{a, a.Me, a.H, a.Z});
        CHECK_LAUNCH();
    }
    a.dbg = next_dbg(c);
    pr.mark(K_P4_DECOUT);
    REP(pr) launch_decout(c, s, a);
    CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------ the training step
// 16-byte dhd operand loads (PDhdT<true>): D % 4 == 0 and 16-byte aligned dA2 / W2 (the
// Gaussian halves dA6 / W6 then are too: they sit a multiple of 4 elements further).
bool dhd_vec(const StepArgs& a) { return (a.D & 3) == 0 && aligned16(a.dA2) && aligned16(a.W2); }

// The dhd launch's arguments, for the folded form (dhd_dz_wgrad_kernel) and the plain one
// (tile_wgrad_kernel) alike: P5 + dW2 (| dW6) = [hd|1]^T [dA2 (| dA6)] in one grid, both need
// only P4's outputs.  The dhd tiles are blocks [0, ntile), gx of them per tile row; the dW2
// tiles (w) follow.
struct DhdLaunch {
    PDhdT<true> p5;     // 16-byte operand loads (vec)
    PDhdT<false> p5s;   // scalar loads
    int gx, ntile;
    WGradArgs w;
    bool vec, deep;
};
int dhd_args(vaeb_ctx* c, const StepArgs& a, const OptArgs& opt, DhdLaunch& d) {
    const int K = gaussian(c) ? ((a.D + 3) & ~3) + a.D : a.D;
    d.p5 = PDhdT<true>{a, a.Me, a.H, K};
    d.p5s = PDhdT<false>{a, a.Me, a.H, K};
    d.gx = cdiv(a.Me, 16);
    d.ntile = d.gx * cdiv(a.H, 16);
    if (int rc = w2_args(c, a, opt, d.ntile, d.w, d.vec)) return rc;
    // the dhd loaders' 16-byte form needs D % 4 == 0 and aligned dA2 / W2 too
    d.vec = d.vec && dhd_vec(a);
    d.deep = chunk_group(K) == 8;
    return 0;
}

// One fp32 training step reading parameter arena `par` and writing arena par ^ 1.
// One stream: P1 -> P23 -> P4 -> [P5 | dW2 (| dW6)] -> [P67 | dW1] -> [dW3 | dW45 + ELBO]
// (bracketed groups share one grid, see hfuse.hpp); DP adds all-reduce -> Adagrad.
// `prof` brackets every launch with timing events.
// fresh: first step of an enqueued sequence (VAEB_EST_FVS in Philox mode draws the weight
// sample here; later steps of the sequence read the one their predecessor's update wrote).
// direct >= 0: the step's minibatch index given by the host (vaeb_update's single eager
// step): the rows are addressed from the launch arguments, no order upload, no cursor.
int enqueue_train_step_f32(vaeb_ctx* c, int par, bool prof, bool fresh, int direct) {
    Prof pr{c, prof};
    if (prof) pr.reps = c->prof_reps;
    const vaeb_config& g = c->c;
    const ArenaSlots& sl = c->sl;
    hipStream_t s = c->s;
    // VAEB_EST_FVS: the step reads the weight sample theta~ written into the spare arena
    // par ^ 1 (the loaded theta in arena par is never updated, as on the literal path)
    const bool fvs = g.estimator == VAEB_EST_FVS;
    const float* zin = (fvs && c->eps_mode == VAEB_EPS_HOST) ? c->fvzeta : nullptr;
    if (fvs && (fresh || zin)) {
        pr.mark(K_FVS_SAMPLE);
        REP(pr) hipLaunchKernelGGL(fvs_sample_kernel, dim3(kFvParts), dim3(256), 0, s, c->fvmu, c->fvsg,
                                   c->theta2[par ^ 1], c->P, c->seed, c->step, zin);
        CHECK_LAUNCH();
    }
    if (fvs) par ^= 1;
    StepArgs a = make_args(c, par, g.B, g.estimator == VAEB_EST_FV ? MODE_EVAL : MODE_TRAIN, c->data, true);
    if (direct >= 0) {
        const int64_t row0 = (int64_t)direct * g.B_global + g.row_offset;
        a.order = nullptr;
        a.xbase = c->data + row0 * g.D;
        a.batch_stride = 0;
        a.row_base_mul = 0;
        a.row_base_add = row0;
    }
    // literal FV: the (mu, sigma) update needs none of the step's data; with the folded
    // latent block it rides enc_latent_kernel's extra grid rows (~256 blocks), else it is
    // fv_kernel's launch
    const bool fv_fold = g.estimator == VAEB_EST_FV && folded_latent(c, a);
    int n_fv = kFvParts;
    FvFold fvf{};
    if (fv_fold) {
        fvf = FvFold{c->fvmu, c->fvsg, c->fvam, c->fvas, c->fv_part, c->P, g.lr, g.adagrad_eps, cdiv(256, a.Mbp / 16)};
        n_fv = fvf.rows * (a.Mbp / 16);
        if (n_fv > kFvParts) return fail(VAEB_ERR_ARG, "internal: %d FV partials > %d", n_fv, kFvParts);
    }
    // the deferred dW2: the PREVIOUS step's dW2 (| dW6) rides this step's encoder launch --
    // theta from the other arena, theta' into this step's (make_opt(par ^ 1)); this step's own
    // dW2 is left pending for the next step (or a flush)
    const bool w2d = dw2_deferred(c, a);
    W2Launch w2{};
    if (w2d) {
        const W2Plan pl = w2_plan_for(c, a);
        w2.width = pl.width;
        w2.paired = pl.paired != 0;
        if (int rc = w2_args(c, a, make_opt(c, par ^ 1, true, g.keep_grads != 0), 0, w2.w, w2.vec, pl.width)) return rc;
        if (pl.width == 64 && !w2.vec) return fail(VAEB_ERR_ARG, "internal: 64-wide dW2 tiles need 16-byte accesses");
        // (timeline build: the dW2 tiles stamp at logical ids 256 + tile of the encoder launch)
        w2.w.dbg = c->dbg ? c->dbg + (size_t)c->dbg_slot * kDbgWG * 8 + 256 * 8 : nullptr;
        w2.pend = c->w2pend;
    }
    if (int rc = enqueue_forward(c, a, pr, fvf, w2d ? &w2 : nullptr)) return rc;
    ElboArgs e = base_elbo(c, a);
    e.elbo_out = c->elbo_out; e.epoch = c->epoch; e.cursor = direct >= 0 ? nullptr : c->ictl; e.step = c->step;
    // the FV estimators' closing launch: SGVB = B (sum log p + sum KL) + thetaPrior (VAEB.py:364)
    auto fv_elbo = [&](int n_parts) {
        pr.mark(K_ELBO);
        e.fv_part = c->fv_part; e.n_fv = n_parts;
        e.data_mul = (double)g.B;
        e.est = VAEB_EST_FV;
        hipLaunchKernelGGL(elbo_kernel, dim3(1), dim3(256), 0, s, e);
    };

    if (g.estimator == VAEB_EST_FV) {
        if (!fv_fold) {
            pr.mark(K_FV_UPDATE);
            REP(pr) hipLaunchKernelGGL(fv_kernel, dim3(kFvParts), dim3(256), 0, s, c->fvmu, c->fvsg, c->fvam,
                                       c->fvas, c->P, g.lr, g.adagrad_eps, 1, c->fv_part);
            CHECK_LAUNCH();
        }
        fv_elbo(n_fv);
        CHECK_LAUNCH();
        pr.mark(K_END);
        c->prof_n = pr.k;
        return 0;
    }
    const bool dp = c->comm != nullptr;  // any communicator (also world 1) takes the all-reduce path
    // FVS: the weight-gradient launches only store the data gradient at theta~
    const OptArgs opt = make_opt(c, par, !dp && !fvs, dp || fvs || g.keep_grads != 0);
    const OptArgs dopt = make_opt(c, par, true, false);
    auto dp_opt = [&](hipStream_t st, const DpRange& r) -> int { return dp_opt_launch(c, st, dopt, r, e); };

    // folded latent backward (Z <= 32, latent_bwd.hpp): the dhd launch also finishes dZ and
    // [dMu | dLv]; dA3 is formed inside the dW3 workgroups of the last launch (with dW1)
    const bool fold = fused_latent(c) && c->fold_bwd;
    a.dbg = next_dbg(c);
    DhdLaunch d{};
    if (int rc = dhd_args(c, a, opt, d)) return rc;
    if (fold) {
        DhdAux pend{nullptr};
        if (w2d) {   // no dW2 tiles here: the next step's encoder launch (or a flush) runs them
            d.w.total_wgs = d.ntile;
            pend.pend = c->w2pend;
        }
        const dim3 grid(d.w.total_wgs);
        pr.mark(w2d ? K_P5_DHD_DZ : K_P5_DHD_DZ_W2);
        REP(pr) if (!dispatch<0, 1, 2>(ho_dz(c), [&](auto HO) {
            launch_dhd_dz<kWTJ_P5 / 16, decltype(HO)::value>(s, grid, d.p5, d.p5s, d.w, d.ntile, d.gx, d.vec, d.deep, pend);
        })) return fail(VAEB_ERR_ARG, "internal: no dhd launch for backward hand-off %d", ho_dz(c));
        CHECK_LAUNCH();
        if (w2d) c->w2_dirty = true;
    } else {
        const dim3 grid(d.w.total_wgs);
        pr.mark(K_P5_DHD_W2);
        REP(pr) dispatch<4, 8>(d.deep ? 8 : 4, [&](auto GCH) {
            constexpr int gch = decltype(GCH)::value, ts = kWTJ_P5 / 16;
            if (d.vec) hipLaunchKernelGGL((tile_wgrad_kernel<1, 1, 8, 1, gch, PDhdT<true>, true, ts>), grid, dim3(512), 0, s, d.p5, d.w, d.ntile, d.gx);
            else hipLaunchKernelGGL((tile_wgrad_kernel<1, 1, 8, 1, gch, PDhdT<false>, false, ts>), grid, dim3(512), 0, s, d.p5s, d.w, d.ntile, d.gx);
        });
        CHECK_LAUNCH();
    }
    auto no_fix = [](hipStream_t, const DpRange&) -> int { return 0; };
    if (dp) if (int rc = dp_bucket_a(c, pr, dopt.theta_out, dp_opt, no_fix)) return rc;
    const WGroup g1w = make_group(c, c->z, a.Z, a.Me, 0, a.Z, c->dA1, a.H, a.H, nullptr, 0, 0, a.Me, sl.W1, sl.b1, -1, -1);
    // P67 (+ dW1 = [z|1]^T dA1 on the fused path): both need only P5's output
    if (!fold) {
        a.dbg = next_dbg(c);
        if (fused_latent(c)) {
            const int nrow = a.Mbp / 16 * std::max(1, std::min(kDzSplit, cdiv(a.H, 16)));
            WGradArgs w;
            bool vec;
            if (int rc = prep_wgrad(c, &g1w, 1, opt, nullptr, a, nrow, w, vec, kWTJ_P67)) return rc;
            const dim3 grid(w.total_wgs);
            pr.mark(K_P67_DZ_DH_W1);
            REP(pr) dispatch<1, 2>(latent_tiles(a), [&](auto NCT) {
                dispatch<false, true>(vec, [&](auto VEC) {
                    hipLaunchKernelGGL((dz_dh_wgrad_kernel<decltype(NCT)::value, decltype(VEC)::value, kWTJ_P67 / 16>), grid,
                                       dim3(512), 0, s, a, w, nrow);
                });
            });
            CHECK_LAUNCH();
        } else {
            pr.mark(K_P8_WGRAD_W1);
            REP(pr) if (int rc = launch_wgrad(c, s, &g1w, 1, opt, nullptr, a)) return rc;
            a.dbg = next_dbg(c);
            pr.mark(K_P6_DZ);
            REP(pr) launch_tile<1, 1, 4, 1, 8>(s, PDz{a, a.Me, a.Z, a.H});
            CHECK_LAUNCH();
            a.dbg = next_dbg(c);
            pr.mark(K_P7_DH);
            REP(pr) launch_tile<1, 4, 1, 1, 8>(s, PDh{a, a.Mbp, a.H, 2 * a.Z});
            CHECK_LAUNCH();
        }
    }
    // dW3 = [X|1]^T dA3 and dW4|dW5 = [h|1]^T [dMu|dLv] (+ dW1 = [z|1]^T dA1 when the latent
    // backward is folded: dA3 is then formed in the dW3 workgroups), plus the ELBO workgroup
    {
        WGroup g12[3] = {
            make_group(c, nullptr, a.D, a.Mb, 1, a.D, c->dA3, a.H, a.H, nullptr, 0, 0, a.Mbp, sl.W3, sl.b3, -1, -1),
            make_group(c, c->h, a.H, a.Mbp, 0, a.H, c->dMuLv, 2 * a.Z, a.Z, c->dMuLv + a.Z, 2 * a.Z, a.Z, a.Mbp, sl.W4,
                       sl.b4, sl.W5, sl.b5),
            g1w};
        ElboArgs e1 = e;
        if (dp || fvs) { e1.dp_slot = c->grad + c->P; e1.elbo_out = nullptr; e1.cursor = nullptr; e1.step = nullptr; }
        a.dbg = next_dbg(c);
        if (fold) {
            Da3Src d3{c->dMuLv, a.W4, a.W5, c->h, c->dA3, a.Z, a.H, a.Mb, a.Mbp, LatRed{}};
            if (ho_dz(c) == 2) {
                // the deferred latent backward: ceil(Z / 8) column groups per 16-row block
                LatRed& r = d3.red;
                r.slab = c->slab_dz; r.mu = c->mu; r.lv = c->lv; r.eps = c->eps; r.z = c->z;
                r.dZ = c->dZ; r.dml = c->dMuLv; r.cnt = c->cnt_dz; r.guard = c->blk + kBlkFxErr;
                // (Z % 4 == 0: groups of a multiple of 4 latents, so VAEB_LAT_ST4 reducers can
                // publish whole 16-byte runs; MNIST-20: 8, 8, 4)
                r.ngrp = cdiv(a.Z, 8); r.zg = cdiv(a.Z, r.ngrp);
                if (a.Z % 4 == 0) { r.zg = (r.zg + 3) & ~3; r.ngrp = cdiv(a.Z, r.zg); }
                r.nred = (a.Mbp / 16) * r.ngrp;
                r.nctH = cdiv(a.H, 16); r.L = a.L; r.est = a.est; r.Mb = a.Mb; r.Mbp = a.Mbp; r.Z = a.Z; r.sc = a.sc;
            }
            pr.mark(K_P8_WGRAD_W3W45W1);
            REP(pr) if (int rc = launch_wgrad(c, s, g12, 3, opt, &e1, a, &d3)) return rc;
        } else {
            pr.mark(K_P8_WGRAD_W3W45);
            REP(pr) if (int rc = launch_wgrad(c, s, g12, 2, opt, &e1, a)) return rc;
        }
    }
    if (fvs) {   // Adagrad on (mu_theta, sigma_theta), then the step's SGVB / B and cursor++
        pr.mark(K_FVS_UPDATE);
        REP(pr) hipLaunchKernelGGL(fvs_update_kernel, dim3(kFvParts), dim3(256), 0, s, c->fvmu, c->fvsg, c->fvam,
                                   c->fvas, (const float*)c->grad, c->P, (float)g.B, g.lr, g.adagrad_eps, c->seed,
                                   (const int64_t*)c->step, zin, c->fv_part, zin ? nullptr : c->theta2[par]);
        CHECK_LAUNCH();
        fv_elbo(kFvParts);
        CHECK_LAUNCH();
    }
    if (dp) if (int rc = dp_bucket_b(c, pr, K_ADAGRAD, dopt.theta_out, dp_opt, no_fix)) return rc;
    pr.mark(K_END);
    c->prof_n = pr.k;
    return 0;
}

// ------------------------------------------------------------------ evaluation chunks
// One fp32 chunk: `rows` device rows at x = global rows [r0, r0 + rows).  MODE_EVAL adds
// the chunk's SGVB into eval_acc; MODE_RECON copies the decoder means to out_y (host).
int eval_chunk_f32(vaeb_ctx* c, int epar, const float* x, int rows, int64_t r0, int mode, float* out_y,
                   float* out_lv = nullptr) {
    const vaeb_config& g = c->c;
    StepArgs a = make_args(c, epar, rows, mode, x, false);
    a.row_base_add = r0;
    a.eps_in = c->eps_in ? c->eps_in + r0 * g.Z : nullptr;
    a.eps_in_ld = c->eps_rows;
    Prof pr{c, false};
    if (int rc = enqueue_forward(c, a, pr)) return rc;
    if (mode == MODE_RECON) {
        HIP_TRY(hipMemcpyAsync(out_y, c->y, sizeof(float) * (size_t)rows * g.D, hipMemcpyDeviceToHost, c->s));
        if (out_lv)
            HIP_TRY(hipMemcpyAsync(out_lv, c->dA6, sizeof(float) * (size_t)rows * g.D, hipMemcpyDeviceToHost, c->s));
    } else {
        ElboArgs e = base_elbo(c, a);
        e.eval_acc = c->eval_acc;
        hipLaunchKernelGGL(elbo_kernel, dim3(1), dim3(256), 0, c->s, e);
        CHECK_LAUNCH();
    }
    return 0;
}

// One posterior draw of one fp32 chunk (vaeb_reconstruct_full, n_samples > 0): the decoder outputs
// at z = mu + exp(lv / 2) eps in c->y (| c->dA6), one plane.  eps: the Philox stream of `domain`
// (sample s: 1 | (s + 1) << 1), or in host eps mode the pushed rows from eps_in (the sample's row
// r0; null when nothing was pushed).
int sample_chunk_f32(vaeb_ctx* c, int epar, const float* x, int rows, int64_t r0, uint32_t domain, const float* eps_in) {
    StepArgs a = make_args(c, epar, rows, MODE_RECON, x, false);
    a.L = 1; a.Me = a.Mbp;
    a.eps_mode = c->eps_mode == VAEB_EPS_HOST ? 1 : 0;
    a.domain = domain;
    a.row_base_add = r0;
    a.eps_in = eps_in; a.eps_in_ld = c->eps_rows;
    Prof pr{c, false};
    return enqueue_forward(c, a, pr);
}

// The decoder of one fp32 chunk at the caller's latents (vaeb_decode): `rows` host rows z [rows x Z]
// staged into c->z, then hd, the means to out_mu and (Gaussian decoder, when asked for) the
// log-sigma head to out_lv (host).
int decode_chunk_f32(vaeb_ctx* c, int epar, const float* z, int rows, float* out_mu, float* out_lv) {
    const vaeb_config& g = c->c;
    StepArgs a = make_args(c, epar, rows, MODE_RECON, c->xeval, false);
    a.L = 1; a.Me = a.Mbp;
    // z rows, pad rows zero (PDecHid writes hd = 0 there)
    HIP_TRY(hipMemsetAsync(c->z, 0, sizeof(float) * (size_t)a.Mbp * g.Z, c->s));
    HIP_TRY(hipMemcpyAsync(c->z, z, sizeof(float) * (size_t)rows * g.Z, hipMemcpyHostToDevice, c->s));
    launch_tile<1, 4, 1, 1, 8>(c->s, PDecHid{a, a.Me, a.H, a.Z});
    CHECK_LAUNCH();
    if (gaussian(c)) launch_bigk<2>(c->s, PDecOut{a, nullptr, a.Me, a.D, a.H});
    else launch_bigk<1>(c->s, PDecOut{a, nullptr, a.Me, a.D, a.H});
    CHECK_LAUNCH();
    HIP_TRY(hipMemcpyAsync(out_mu, c->y, sizeof(float) * (size_t)rows * g.D, hipMemcpyDeviceToHost, c->s));
    if (out_lv) HIP_TRY(hipMemcpyAsync(out_lv, c->dA6, sizeof(float) * (size_t)rows * g.D, hipMemcpyDeviceToHost, c->s));
    return 0;
}

// The encoder and heads of one fp32 chunk (rows at x = global rows [r0, r0 + rows)): c->mu and
// c->lv hold it afterwards (VAEB.py:245-251).  The forward's own launches with zero noise and
// one plane; what they also write (eps, z, hd plane 0, the KL partials) is scratch here.
int encode_chunk_f32(vaeb_ctx* c, int epar, const float* x, int rows, int64_t r0, StepArgs* out) {
    StepArgs a = make_args(c, epar, rows, MODE_EVAL, x, false);
    a.L = 1; a.Me = a.Mbp;
    a.est = EST_LB;
    a.eps_mode = 2;
    a.row_base_add = r0;
    launch_bigk<1>(c->s, PEnc{a, nullptr, a.Mbp, a.H, a.D});
    CHECK_LAUNCH();
    if (fused_latent(c)) launch_heads_dechid(c->s, a);
    else launch_tile<1, 1, 4, 2, 8>(c->s, PHeads{a, a.Mbp, a.Z, a.H});
    CHECK_LAUNCH();
    if (out) *out = a;
    return 0;
}

// IW_K of one chunk (iwae.hpp): `rows` device rows at x = global rows [r0, r0 + rows); eps_k0:
// host eps mode, sample 0's noise row of the chunk's row 0 (sample k is eps_ld rows further).
// Adds the chunk's sum to eval_acc[0]; the row values go to out_rows (host) when given.
int iw_chunk_f32(vaeb_ctx* c, int epar, const float* x, int rows, int64_t r0, int K, const float* eps_k0,
                 int64_t eps_ld, float* out_rows) {
    const vaeb_config& g = c->c;
    StepArgs a;
    if (int rc = encode_chunk_f32(c, epar, x, rows, r0, &a)) return rc;
    const int64_t planes = (int64_t)c->cap * g.L;   // rows of z / hd / lp_part
    IwArgs w{};
    w.Z = g.Z; w.Mb = rows; w.Mbp = a.Mbp; w.nctD = a.nctD;
    w.K = K; w.logK = (float)std::log((double)K);
    w.row0 = r0;
    w.eps_mode = c->eps_mode == VAEB_EPS_HOST ? 1 : 0;
    w.seed = c->seed; w.step = c->step;
    w.eps_in = eps_k0; w.eps_ld = eps_ld;
    w.mu = c->mu; w.lv = c->lv; w.z = c->z; w.lp_part = c->lp_part;
    w.lat = c->iw; w.ms = c->iw + planes; w.rows = w.ms + 2 * (int64_t)c->cap;
    const int smax = (int)std::min<int64_t>(planes / a.Mbp, K);
    for (int k0 = 0; k0 < K; k0 += smax) {
        const int S = std::min(smax, K - k0);
        w.k0 = k0; w.S = S;
        hipLaunchKernelGGL(iw_sample_kernel, dim3((unsigned)(S * (a.Mbp / 16))), dim3(256), 0, c->s, w);
        CHECK_LAUNCH();
        StepArgs d = a;
        d.L = S; d.Me = S * a.Mbp;
        launch_tile<1, 4, 1, 1, 8>(c->s, PDecHid{d, d.Me, d.H, d.Z});
        CHECK_LAUNCH();
        launch_decout(c, c->s, d);
        CHECK_LAUNCH();
        hipLaunchKernelGGL(iw_lse_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, c->s, w);
        CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(iw_sum_kernel, dim3(1), dim3(256), 0, c->s, w.rows, (int64_t)rows, c->eval_acc);
    CHECK_LAUNCH();
    if (out_rows) HIP_TRY(hipMemcpyAsync(out_rows, w.rows, sizeof(float) * (size_t)rows, hipMemcpyDeviceToHost, c->s));
    return 0;
}
