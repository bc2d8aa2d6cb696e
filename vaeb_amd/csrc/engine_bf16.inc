// engine_bf16.inc -- host orchestration of the bf16 large-batch step (step_bf16.hpp).
// Included by vaeb_hip.hip inside its anonymous namespace, after the fp32 helpers.

// Instantiated twice by vaeb_hip.hip: namespace eng_bf (bf = vaeb::bf, bf16 operands) and
// eng_hf (bf = vaeb::hf, fp16 operands), kF16 telling them apart (h16_engines.hpp).

using bf::bf16_t;

// The backward's loss scale S (fp16 only).  The mean objective (VAEBfullbayes.py:142) scales
// every data gradient by 1 / B_global: at config-5 sizes dA1, dZ and [dMu | dLv] then fall below
// fp16's smallest normal (6.1e-5) and lose their mantissa bits.  The fp16 engine stores the
// backward's 16-bit operands scaled by S, the largest power of two <= B_global (exact; the
// sum-objective magnitudes at most), and every fp32 weight-gradient epilogue multiplies by
// 1 / S (bf::Opt::gs), so the stored gradients, the Adagrad state and theta are those of the
// unscaled step.  bf16 keeps fp32's exponent range, and the sum objective's gradients are
// O(1): S = 1 there.
float h16_scale(const vaeb_ctx* c) {
    if (!kF16 || c->c.objective != VAEB_OBJ_MEAN_MAP) return 1.f;
    int e2 = 0;
    std::frexp((float)c->c.B_global, &e2);   // B_global = m 2^e2, m in [0.5, 1)
    return std::ldexp(1.f, e2 - 1);
}

// fp16: the guard word that a training step's range-checked 16-bit stores report to
// (h16_engines.hpp, H16_GUARD_FIELD); the bf16 structs have no such member.
template <class E>
E h16_guarded(vaeb_ctx* c, E e, bool train = true) {
    if constexpr (kF16) {
        if (train) e.guard = c->blk + kBlkFxErr;
    }
    return e;
}

// Block-tile width for an M x N product: 256-wide tiles unless that leaves the chip
// (256 CUs, one block each) less than full.
int bf_bn(int M, int N) { return cdiv(M, bf::BM) * cdiv(N, 256) >= 256 ? 256 : 128; }


template <int LA, int LB, class E>
int bf_launch8(hipStream_t s, const bf::GemmArgs& g, int nz, const E& e) {
    static bool attr_set = false;
    constexpr int lds = bf::lds8_bytes();
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)bf::gemm8_kernel<LA, LB, E>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    lds));
        attr_set = true;
    }
    hipLaunchKernelGGL((bf::gemm8_kernel<LA, LB, E>), dim3(g.tiles_m * g.tiles_n, nz), dim3(bf::NTHR), lds, s, g, e);
    CHECK_LAUNCH();
    return 0;
}

template <int LA, int LB, int BNT, class E, int ST = 4>
int bf_launch(hipStream_t s, const bf::GemmArgs& g, int nz, const E& e) {
    // (the Gaussian decoder's epilogue pairs fragment tiles 32 columns apart: gemm_body only)
    if constexpr (BNT == 256 && ST == 4 && !std::is_same_v<E, bf::EpiDecOut<true>>) {
        if (use8<LA, LB>()) return bf_launch8<LA, LB, E>(s, g, nz, e);
    }
    static bool attr_set = false;   // one per instantiation: > 64 KiB of dynamic LDS
    constexpr int lds = bf::lds_bytes<BNT, ST>();
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)bf::gemm_kernel<LA, LB, BNT, E, ST>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_set = true;
    }
    hipLaunchKernelGGL((bf::gemm_kernel<LA, LB, BNT, E, ST>), dim3(g.tiles_m * g.tiles_n, nz), dim3(bf::NTHR), lds, s, g, e);
    CHECK_LAUNCH();
    return 0;
}

// thin_bf16.hpp launches (> 64 KiB of dynamic LDS)
template <int LB, int BMT, class E>
int bf_thin(hipStream_t s, const bf::ThinArgs& t, dim3 grid, const E& e) {
    static bool attr_set = false;
    constexpr int lds = bf::ThinShape<BMT>::kSmem;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)bf::thin_kernel<LB, BMT, E>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_set = true;
    }
    hipLaunchKernelGGL((bf::thin_kernel<LB, BMT, E>), grid, dim3(bf::NTHR), lds, s, t, e);
    CHECK_LAUNCH();
    return 0;
}

template <int LA, int LB, class E>
int bf_gemm(hipStream_t s, const bf16_t* A, int lda, int64_t a_bytes, const bf16_t* B, int ldb,
            int64_t b_bytes, int M, int N, int K, int ks, const E& e, bf::BatchRef ab = bf::BatchRef{}) {
    bf::GemmArgs g{};
    g.A = A; g.lda = lda; g.a_bytes = a_bytes; g.ab = ab;
    g.B = B; g.ldb = ldb; g.b_bytes = b_bytes;
    g.M = M; g.N = N; g.K = K;
    const int bn = bf_bn(M, N);
    g.tiles_m = cdiv(M, bf::BM); g.tiles_n = cdiv(N, bn);
    ks = std::max(1, ks);
    g.kslice = ((cdiv(K, ks) + bf::BK - 1) / bf::BK) * bf::BK;
    const int nz = cdiv(K, g.kslice);
    if (bn == 256) return bf_launch<LA, LB, 256>(s, g, nz, e);
    return bf_launch<LA, LB, 128>(s, g, nz, e);
}

// Two products in one 256 x 256-tile grid (gemm2_kernel): product 1's blocks first.
template <int LA1, int LB1, class E1, int LA2, int LB2, class E2>
int bf_gemm2(hipStream_t s, const bf::GemmArgs& g1, const E1& e1, const bf::GemmArgs& g2, const E2& e2) {
    if (use8<LA1, LB1>() && use8<LA2, LB2>()) {
        static bool attr8 = false;
        constexpr int lds8 = bf::lds8_bytes();
        auto k8 = bf::gemm8x2_kernel<LA1, LB1, E1, LA2, LB2, E2>;
        if (!attr8) {
            HIP_TRY(hipFuncSetAttribute((const void*)k8, hipFuncAttributeMaxDynamicSharedMemorySize, lds8));
            attr8 = true;
        }
        const int nb1 = g1.tiles_m * g1.tiles_n, nb2 = g2.tiles_m * g2.tiles_n;
        hipLaunchKernelGGL(k8, dim3(nb1 + nb2), dim3(bf::NTHR), lds8, s, g1, e1, g2, e2, nb1);
        CHECK_LAUNCH();
        return 0;
    }
    static bool attr_set = false;
    constexpr int lds = bf::lds_bytes<256>();
    auto kern = bf::gemm2_kernel<LA1, LB1, E1, LA2, LB2, E2, 256>;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_set = true;
    }
    const int nb1 = g1.tiles_m * g1.tiles_n, nb2 = g2.tiles_m * g2.tiles_n;
    hipLaunchKernelGGL(kern, dim3(nb1 + nb2), dim3(bf::NTHR), lds, s, g1, e1, g2, e2, nb1);
    CHECK_LAUNCH();
    return 0;
}

// A short-K product (dechid K = Z, dh K = 2Z) on 256 x 128 tiles with the 3-stage ring and
// two blocks per CU, so one block's epilogue (activation, tile stores) overlaps the other's
// loads instead of running after them (the 256 x 256 tile does both in series).
template <int LA, int LB, class E>
int bf_gemm_2b(hipStream_t s, const bf16_t* A, int lda, int64_t a_bytes, const bf16_t* B, int ldb, int64_t b_bytes,
               int M, int N, int K, const E& e, bf::BatchRef ab = bf::BatchRef{}) {
    bf::GemmArgs g{};
    g.A = A; g.lda = lda; g.a_bytes = a_bytes; g.ab = ab;
    g.B = B; g.ldb = ldb; g.b_bytes = b_bytes;
    g.M = M; g.N = N; g.K = K;
    g.tiles_m = cdiv(M, bf::BM); g.tiles_n = cdiv(N, 128);
    g.kslice = ((K + bf::BK - 1) / bf::BK) * bf::BK;
    return bf_launch<LA, LB, 128, E, 3>(s, g, 1, e);
}

// GemmArgs of one product on 256 x 256 tiles, whole K in one slice.
bf::GemmArgs bf_args256(const bf16_t* A, int lda, int64_t a_bytes, const bf16_t* B, int ldb, int64_t b_bytes, int M,
                        int N, int K, int slices = 1, bf::BatchRef ab = bf::BatchRef{}) {
    bf::GemmArgs g{};
    g.A = A; g.lda = lda; g.a_bytes = a_bytes; g.ab = ab;
    g.B = B; g.ldb = ldb; g.b_bytes = b_bytes;
    g.M = M; g.N = N; g.K = K;
    g.tiles_m = cdiv(M, bf::BM); g.tiles_n = cdiv(N, 256);
    g.kslice = ((cdiv(K, slices) + bf::BK - 1) / bf::BK) * bf::BK;
    return g;
}

// Rows of the epilogues' column-partial arrays for M GEMM rows: one per 64-row wave block
// of every row tile (the empty ones write zeros).
int bf_rowblocks(int64_t M) { return cdiv(M, bf::BM) * (bf::BM / 64); }
// The same for EpiDTanhT, whose output rows are the product's N' = rows (its M' = cols): four
// wave slots per 256-row tile (gemm8, Col8) or two per 128-row tile (the ring, ColStd).
int bf_rowblocks_t(int rows, int cols) { return bf_bn(cols, rows) == 256 ? cdiv(rows, 256) * 4 : cdiv(rows, 128) * 2; }

// Split-K slices so that a thin product still puts >= ~256 blocks on the chip, keeping
// >= 4 K tiles per slice.
int bf_split(int M, int N, int K) {
    const int tiles = cdiv(M, bf::BM) * cdiv(N, bf_bn(M, N));
    int ks = cdiv(256, tiles);
    ks = std::min(ks, std::max(1, K / (4 * bf::BK)));
    return std::max(1, ks);
}
int bf_slices(int K, int ks) {
    const int kslice = ((cdiv(K, ks) + bf::BK - 1) / bf::BK) * bf::BK;
    return cdiv(K, kslice);
}

// A KO x KO weight gradient on full-depth 256 x 256 tiles.  (Running it as two K slices
// combined in the launch -- split2_combine, 1096-1127 TF/s bare -- measured slower in the forked
// step, 821 vs 801 us in round 4, where dW2 and dW3 already share the chip; the step switch
// VAEB_BF_SPLIT2 was removed in round 6, the kernel form stays for vaeb_test_gemm_bf16 /
// vaeb_bench_gemm_bf16.)
template <class E>
int bf_wgrad256(hipStream_t s, const bf::GemmArgs& g, const E& e) {
    return bf_launch<bf::KO, bf::KO, 256>(s, g, 1, e);
}

int bf_alloc(vaeb_ctx* c) {
    bf::BfState& b = c->bf;
    const vaeb_config& g = c->c;
    const int D = g.D, H = g.H, Z = g.Z, L = g.L;
    const bool gs = gaussian(c);
    b.on = true;
    b.Dn = gs ? 2 * D : D;
    b.s3 = 0;
    b.s45 = (int64_t)D * H;
    b.s1 = b.s45 + (int64_t)H * 2 * Z;
    b.s26 = b.s1 + (int64_t)Z * H;
    b.S = b.s26 + (int64_t)H * b.Dn;
    bf::ShadowMap& m = b.smap;
    const ArenaSlots& sl = c->sl;
    m.offW3 = c->off[sl.W3]; m.offW4 = c->off[sl.W4]; m.offW5 = c->off[sl.W5]; m.offW1 = c->off[sl.W1];
    m.offW2 = c->off[sl.W2];
    m.offW6 = gs ? c->off[sl.W6] : -1;
    m.s3 = b.s3; m.s45 = b.s45; m.s1 = b.s1; m.s26 = b.s26;
    m.D = D; m.H = H; m.Z = Z;
    m.nweights = c->off[sl.b3];   // the biases follow the weight matrices
    const int64_t R = c->cap, RL = (int64_t)c->cap * L;
    const int B = g.B;
    b.ks_heads = bf_split(B, 2 * Z, H);
    // dz's slabs are re-read by latent_bwd: keep >= 16 K tiles per slice (config 5: 4 slices
    // instead of 8; latent_bwd 9.6 -> 6.2 us, dz 15.0 -> 17.3 us, step 821-822 -> 817-819 us)
    b.ks_dz = std::max(1, std::min(bf_split(L * B, Z, H), H / (16 * bf::BK)));
    // A/B: fewer split-K slices for the latent-width products (fewer blocks, longer K per
    // block, less fp32 slab traffic for the latent kernels to read)
    b.ks_w1 = bf_split(Z, H, L * B);
    b.ks_w45 = bf_split(H, 2 * Z, B);
    const int64_t nrbL = bf_rowblocks(RL) + 1;
    const bool thin_ok = Z % 128 == 0 && L == 1 && g.estimator == VAEB_EST_LB && H % 8 == 0;
    b.thin_h = thin_ok && (c->bf_thin & 1);
    b.thin_z = thin_ok && (c->bf_thin & 2);
    b.nkl = b.thin_h ? Z / 64 : 1;
    int rc = 0;
    rc = rc ? rc : dalloc(&b.shadow2[0], (size_t)b.S);
    rc = rc ? rc : dalloc(&b.shadow2[1], (size_t)b.S);
    rc = rc ? rc : dalloc(&b.xeval, (size_t)R * D);
    rc = rc ? rc : dalloc(&b.h, (size_t)R * H);
    rc = rc ? rc : dalloc(&b.z, (size_t)RL * Z);
    rc = rc ? rc : dalloc(&b.hd, (size_t)RL * H);
    rc = rc ? rc : dalloc(&b.dA, (size_t)RL * b.Dn);
    rc = rc ? rc : dalloc(&b.dA1, (size_t)RL * H);
    rc = rc ? rc : dalloc(&b.dml, (size_t)R * 2 * Z);
    rc = rc ? rc : dalloc(&b.dA3, (size_t)R * H);
    rc = rc ? rc : dalloc(&b.ml_slab, (size_t)b.ks_heads * R * 2 * Z);
    rc = rc ? rc : dalloc(&b.dz_slab, (size_t)std::max(b.ks_dz, cdiv(H, 256)) * RL * Z);   // (dz fused into dhd: H / 256 slabs)
    rc = rc ? rc : dalloc(&b.w_slab, std::max((size_t)b.ks_w1 * Z * H, (size_t)b.ks_w45 * H * 2 * Z));
    rc = rc ? rc : dalloc(&b.cp3, (size_t)nrbL * H);
    rc = rc ? rc : dalloc(&b.cp45, (size_t)(cdiv(R, bf::kLbRows) + 1) * 2 * Z);
    rc = rc ? rc : dalloc(&b.cp1, (size_t)nrbL * H);
    rc = rc ? rc : dalloc(&b.cp26, (size_t)nrbL * b.Dn);
    rc = rc ? rc : dalloc(&b.lp, (size_t)RL * cdiv(b.Dn, 64));
    rc = rc ? rc : dalloc(&b.kl, (size_t)RL * b.nkl);
    rc = rc ? rc : dalloc(&b.mu, (size_t)R * Z);
    rc = rc ? rc : dalloc(&b.lv, (size_t)R * Z);
    rc = rc ? rc : dalloc(&b.eps, (size_t)RL * Z);
    rc = rc ? rc : dalloc(&b.elbo_parts, (size_t)2 * bf::kElboBlocks);
    return rc;
}

void bf_free(vaeb_ctx* c) {
    bf::BfState& b = c->bf;
    void* ps[] = {b.shadow2[0], b.shadow2[1], b.x, b.xbits, b.xeval, b.xval, b.h, b.z, b.hd, b.dA, b.dA1, b.dml, b.dA3, b.ml_slab,
                  b.dz_slab, b.w_slab, b.cp3, b.cp45, b.cp1, b.cp26, b.lp, b.kl, b.mu, b.lv, b.eps,
                  b.elbo_parts};
    for (void* p : ps) if (p) hipFree(p);
    b = bf::BfState{};
}

int bf_make_shadow(vaeb_ctx* c, int par) {
    hipLaunchKernelGGL(bf::make_shadow_kernel, dim3(1024), dim3(256), 0, c->s, c->theta2[par], c->bf.shadow2[par],
                       c->bf.smap);
    CHECK_LAUNCH();
    return 0;
}

// fp32 host rows -> bf16 device rows, through the fp32 eval staging buffer in chunks.
int bf_upload_rows(vaeb_ctx* c, const float* x, int64_t n, bf16_t* dst) {
    const int64_t D = c->c.D;
    const int64_t chunk = (int64_t)c->cap;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t rows = std::min(chunk, n - r0);
        HIP_TRY(hipMemcpyAsync(c->xeval, x + r0 * D, sizeof(float) * (size_t)(rows * D), hipMemcpyHostToDevice, c->s));
        hipLaunchKernelGGL(bf::to_bf16_kernel, dim3(512), dim3(256), 0, c->s, c->xeval, dst + r0 * D, rows * D);
        CHECK_LAUNCH();
    }
    return 0;
}

// The 16-byte latent kernels (step_bf16.hpp *_v4): Z % 4 == 0 and every operand they read
// or write with 16-byte accesses 16-byte aligned (else the 4-byte forms; config 5: +6 us).
bool bf_lat4(const vaeb_ctx*, const bf::LatentArgs& la) {
    if ((la.Z & 3) != 0) return false;
    const void* ps[] = {la.ml_slab, la.b4, la.b5, la.mu, la.lv, la.eps, la.z, la.dz_slab, la.dmulv, la.eps_in};
    for (const void* p : ps)
        if (p && (reinterpret_cast<uintptr_t>(p) & 15) != 0) return false;
    return true;   // row offsets are multiples of Z: 16 B for fp32, 8 B for the bf16 z
}

bf::Opt bf_opt(vaeb_ctx* c, int par, bool update, bool store) {
    const OptArgs o = make_opt(c, par, update, store);
    bf::Opt q{};
    q.th_in = o.theta_in; q.th_out = o.theta_out; q.accum = o.acc; q.grad = o.grad;
    q.shadow_out = c->bf.shadow2[par ^ 1];
    q.lr = o.lr; q.eps = o.eps; q.prior = o.prior; q.decay = o.decay;
    q.update = o.update; q.store_grad = o.store_grad;
    q.n = c->P + 1;
    q.gs = 1.f / h16_scale(c);
    return q;
}

bf::ColMap cmap(int mode, int n0, int64_t off0, int64_t off1, int ld0, int ld1) {
    bf::ColMap m{};
    m.mode = mode; m.n0 = n0; m.off0 = off0; m.off1 = off1; m.ld0 = ld0; m.ld1 = ld1;
    return m;
}

// The Adagrad epilogue's 16-byte form (EpiAdagrad::apply_vec): every four consecutive columns
// of a row are four consecutive arena elements, 16-byte aligned, and four consecutive shadow
// elements, 8-byte aligned
int adagrad_vec(const bf::EpiAdagrad& e) {
    const bf::ColMap& m = e.map;
    auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    bool ok = e.N % 4 == 0 && (e.sld ? e.sld : e.N) % 4 == 0 && m.off0 % 4 == 0 && m.ld0 % 4 == 0;
    if (m.mode != 0) ok = ok && m.off1 % 4 == 0 && m.ld1 % 4 == 0 && m.n0 % 4 == 0;
    ok = ok && a16(e.opt.th_in) && a16(e.opt.th_out) && a16(e.opt.accum) && (!e.opt.store_grad || a16(e.opt.grad));
    ok = ok && (reinterpret_cast<uintptr_t>(e.opt.shadow_out) & 7) == 0;
    return ok ? 1 : 0;
}

int bf_forward(vaeb_ctx* c, int par, const BfFwd& f, Prof& pr) {
    const vaeb_config& g = c->c;
    bf::BfState& b = c->bf;
    hipStream_t s = c->s;
    const int D = g.D, H = g.H, Z = g.Z, L = g.L, M = f.Mb, LM = L * f.Mb, Dn = b.Dn;
    const bf16_t* sh = b.shadow2[par];
    const float* t = c->theta2[par];
    const bool gs = gaussian(c);
    const ArenaSlots& as = c->sl;
    const float *b3 = t + c->off[as.b3], *b4 = t + c->off[as.b4], *b5 = t + c->off[as.b5], *b1 = t + c->off[as.b1],
                *b2 = t + c->off[as.b2], *b6 = gs ? t + c->off[as.b6] : nullptr;
    const int64_t xbytes = (int64_t)M * D * 2;
    // enc: h = tanh(X W3 + b3)
    pr.mark(K_BF_ENC);
    // (256 x 128 tiles with two blocks per CU, as decout: +21 us per step, removed in round 3)
    REP(pr) if (int rc = bf_gemm<bf::KC, bf::KO>(s, f.x, D, xbytes, sh + b.s3, H, (int64_t)D * H * 2, M, H, D, 1,
                                                  bf::EpiBiasAct{b3, 1, M, H, b.h, H}, f.xb)) return rc;
    if (b.thin_h) {
        // heads + latent forward in one launch (thin_bf16.hpp): 64 rows x 64 latents per block
        bf::ThinArgs ta{};
        ta.A = b.h; ta.lda = H; ta.a_bytes = (int64_t)M * H * 2; ta.M = M;
        ta.B = sh + b.s45; ta.ldb = 2 * Z; ta.b_bytes = (int64_t)H * 2 * Z * 2; ta.K = H; ta.bcol1 = Z;
        bf::EpiHeadsLatent eh{};
        eh.b4 = b4; eh.b5 = b5; eh.mu = b.mu; eh.lv = b.lv; eh.eps = b.eps; eh.z = b.z;
        eh.kl_part = b.kl; eh.nkl = b.nkl; eh.M = M; eh.Z = Z; eh.mode = f.mode;
        eh.eps_mode = c->eps_mode == VAEB_EPS_HOST ? 1 : 0; eh.seed = c->seed; eh.step = c->step; eh.domain = f.domain;
        eh.eps_in = f.eps_in; eh.eps_in_ld = f.eps_in_ld;
        eh.rows = f.xb; eh.row_base_mul = f.row_base_mul; eh.row_base_add = f.row_base_add;
        pr.mark(K_BF_HEADS);
        REP(pr) if (int rc = bf_thin<bf::KO, 64>(s, ta, dim3(cdiv(M, 64), Z / 64), h16_guarded(c, eh, f.train))) return rc;
    } else {
    // heads: [mu | lv] split-K slabs
    const int ksh = bf_slices(H, b.ks_heads);
    pr.mark(K_BF_HEADS);
    REP(pr) if (int rc = bf_gemm<bf::KC, bf::KO>(s, b.h, H, (int64_t)M * H * 2, sh + b.s45, 2 * Z,
                                                  (int64_t)H * 2 * Z * 2, M, 2 * Z, H, b.ks_heads,
                                                  bf::EpiF32{b.ml_slab, 2 * Z, M, 2 * Z, (int64_t)M * 2 * Z})) return rc;
    // latent: mu, lv, eps, z, KL / LA terms
    bf::LatentArgs la{};
    la.M = M; la.Z = Z; la.L = L; la.est = g.estimator; la.mode = f.mode;
    la.sc = (g.objective == VAEB_OBJ_MEAN_MAP) ? 1.0f / (float)g.B_global : 1.0f;
    la.ml_slab = b.ml_slab; la.nslab = ksh; la.b4 = b4; la.b5 = b5;
    la.mu = b.mu; la.lv = b.lv; la.eps = b.eps; la.z = b.z; la.kl_part = b.kl;
    la.eps_mode = c->eps_mode == VAEB_EPS_HOST ? 1 : 0; la.seed = c->seed; la.step = c->step; la.domain = f.domain;
    la.eps_in = f.eps_in; la.eps_in_ld = f.eps_in_ld;
    la.rows = f.xb; la.row_base_mul = f.row_base_mul; la.row_base_add = f.row_base_add;
    la = h16_guarded(c, la, f.train);
    pr.mark(K_BF_LATENT);
    if (bf_lat4(c, la)) REP(pr) hipLaunchKernelGGL(bf::latent_fwd_v4_kernel, dim3(cdiv(M, 8)), dim3(256), 0, s, la);
    else REP(pr) hipLaunchKernelGGL(bf::latent_fwd_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, la);
    CHECK_LAUNCH();
    }
    const float lsc = (g.objective == VAEB_OBJ_MEAN_MAP) ? 1.0f / (float)g.B_global : 1.0f;
    // dechid: hd = tanh(z W1 + b1) on 256 x 128 tiles, two blocks per CU (K = Z is short: the
    // second block's epilogue overlaps the first's; 743.3 -> 739.8 us per step in round 5)
    pr.mark(K_BF_DECHID);
    REP(pr) if (int rc = bf_gemm_2b<bf::KC, bf::KO>(s, b.z, Z, (int64_t)LM * Z * 2, sh + b.s1, H, (int64_t)Z * H * 2,
                                                     LM, H, Z, bf::EpiBiasAct{b1, 1, LM, H, b.hd, H})) return rc;
    // decout: log p(x|z) partials, dA2 (| dA6), bias partials, y
    pr.mark(K_BF_DECOUT);
    const int nlp = cdiv(Dn, 64);
    // (dA is stored with the backward's loss scale: the fp16 mean objective, h16_scale)
    const float sl = lsc / (float)L * (f.train ? h16_scale(c) : 1.f);
    if (gs) {
        const bf::EpiDecOut<true> e = h16_guarded(
            c, bf::EpiDecOut<true>{b2, b6, f.x, D, M, LM, Dn, D, f.train ? 1 : 0, sl, f.xb, b.dA, Dn, b.lp, nlp, b.cp26, f.yout},
            f.train);
        REP(pr) if (int rc = bf_gemm<bf::KC, bf::KO>(s, b.hd, H, (int64_t)LM * H * 2, sh + b.s26, Dn,
                                                      (int64_t)H * Dn * 2, LM, Dn, H, 1, e)) return rc;
    } else {
        if (D % 8 == 0 && (reinterpret_cast<uintptr_t>(f.yout) & 15) == 0) {
            // the transposed product a2^T = W2^T hd^T (EpiDecOutT: a lane's four consecutive output
            // columns of one row, 8-byte x / dA accesses through LDS) on the 8-phase 256 x 256
            // tiles, one block per CU (the 256 x 128 two-block form spilled 76 B per lane: 747.6 /
            // 752.2 / 750.4 -> 741.4 / 744.3 / 744.1 us per step, profiles/r5/synth_ab.txt; its
            // switch VAEB_BF_DECT was removed in round 6)
            const bf::EpiDecOutT e = h16_guarded(
                c, bf::EpiDecOutT{b2, f.x, D, M, LM, D, f.train ? 1 : 0, sl, f.xb, b.dA, Dn, b.lp, nlp, b.cp26, f.yout, f.xbits},
                f.train);
            bf::GemmArgs gg = bf_args256(sh + b.s26, Dn, (int64_t)H * Dn * 2, b.hd, H, (int64_t)LM * H * 2, Dn, LM, H);
            REP(pr) if (int rc = bf_launch8<bf::KO, bf::KC>(s, gg, 1, e)) return rc;
        } else {
        // D % 8 != 0: on hd W2, 256 x 128 tiles, 3-stage ring, two blocks per CU (one block's
        // likelihood epilogue beside the other's main loop)
        const bf::EpiDecOut<false> e = h16_guarded(
            c, bf::EpiDecOut<false>{b2, b6, f.x, D, M, LM, Dn, D, f.train ? 1 : 0, sl, f.xb, b.dA, Dn, b.lp, nlp, b.cp26, f.yout},
            f.train);
        bf::GemmArgs gg = bf_args256(b.hd, H, (int64_t)LM * H * 2, sh + b.s26, Dn, (int64_t)H * Dn * 2, LM, Dn, H);
        gg.tiles_n = cdiv(Dn, 128);
        REP(pr) if (int rc = bf_launch<bf::KC, bf::KO, 128, bf::EpiDecOut<false>, 3>(s, gg, 1, e)) return rc;
        }
    }
    return 0;
}

ElboArgs bf_elbo(vaeb_ctx* c, int M) {
    ElboArgs e{};
    const int L = c->c.L;
    e.lp_part = c->bf.lp; e.n_lp = (int64_t)L * M * cdiv(c->bf.Dn, 64);
    e.kl_part = c->bf.kl; e.n_kl = (c->c.estimator == VAEB_EST_LA) ? (int64_t)L * M : (int64_t)M * c->bf.nkl;
    e.L = L; e.est = c->c.estimator;
    e.data_mul = 1.0;
    e.inv_bglob = 1.0 / (double)c->c.B_global;
    return e;
}

// The DP optimizer launch over range r (prior + Adagrad + the bf16 shadow of what it updates;
// r.book: also the SGVB bookkeeping), and the sharded form's shadow rewrite of the elements
// other ranks updated (theta' gathered before it): the step's dp_opt / dp_fix, and what
// vaeb_dp_rank_update runs for one emulated rank.
int bf_dp_opt_launch(vaeb_ctx* c, hipStream_t st, const bf::Opt& o, const DpRange& r, const ElboArgs& e) {
    int64_t n = 0;
    for (int k = 0; k < kDpRuns; ++k) n += r.n[k];
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(r.book ? 1024 : 512, cdiv(n, 256 * 8)));
    hipLaunchKernelGGL(bf::adagrad_bf16_kernel, dim3(nb), dim3(256), 0, st, o, c->P, r, c->bf.smap, e);
    CHECK_LAUNCH();
    return 0;
}
int bf_dp_fix_launch(vaeb_ctx* c, hipStream_t st, const bf::Opt& o, const DpRange& r) {
    int64_t n = 0;
    for (int k = 0; k < kDpRuns; ++k) n += r.n[k];
    if (n == 0) return 0;
    hipLaunchKernelGGL(bf::shadow_runs_kernel, dim3((int)std::min<int64_t>(1024, cdiv(n, 256 * 8))), dim3(256), 0, st,
                       (const float*)o.th_out, o.shadow_out, c->bf.smap, r);
    CHECK_LAUNCH();
    return 0;
}

// One training step: parameters arena par -> par ^ 1.
int bf_train_step(vaeb_ctx* c, int par, bool prof, int direct) {
    Prof pr{c, prof};
    if (prof) pr.reps = c->prof_reps;
    const vaeb_config& g = c->c;
    bf::BfState& b = c->bf;
    hipStream_t s = c->s;
    const int D = g.D, H = g.H, Z = g.Z, L = g.L, M = g.B, LM = L * g.B, Dn = b.Dn;
    const bool gs = gaussian(c);
    const bf16_t* sh = b.shadow2[par];
    // direct >= 0: the host's minibatch index (vaeb_update), rows addressed from the arguments
    const int64_t row0 = direct >= 0 ? (int64_t)direct * g.B_global + g.row_offset : g.row_offset;
    const bf::BatchRef xb = direct >= 0 ? bf::BatchRef{nullptr, nullptr, 0}
                                        : bf::BatchRef{c->ictl + kCtlOrder, c->ictl, (int64_t)g.B_global * D};
    const bf16_t* x0 = b.x + row0 * D;
    int* const cursor = direct >= 0 ? nullptr : c->ictl;

    BfFwd f{};
    f.Mb = M; f.mode = MODE_TRAIN; f.train = true; f.x = x0; f.xb = xb;
    f.row_base_mul = direct >= 0 ? 0 : g.B_global; f.row_base_add = row0;
    f.eps_in = c->eps_in; f.eps_in_ld = c->eps_rows; f.domain = 0; f.yout = nullptr;
    f.xbits = b.xbits ? b.xbits + row0 * (D / 32) : nullptr;
    if (int rc = bf_forward(c, par, f, pr)) return rc;

    const bool dp = c->comm != nullptr;
    const bf::Opt opt = bf_opt(c, par, !dp, dp || g.keep_grads != 0);
    const ArenaSlots& sl = c->sl;
    // DP: replicated Adagrad (+ bf16 shadows) over an all-reduced gradient bucket
    bf::Opt dopt = bf_opt(c, par, true, false);
    dopt.shadow_out = b.shadow2[par ^ 1];
    ElboArgs de = bf_elbo(c, M);
    de.elbo_out = c->elbo_out; de.epoch = c->epoch; de.cursor = cursor; de.step = c->step;
    auto dp_opt = [&](hipStream_t st, const DpRange& r) -> int { return bf_dp_opt_launch(c, st, dopt, r, de); };
    // sharded DP: the shadow of the theta' shards other ranks updated (gathered before it)
    auto dp_fix = [&](hipStream_t st, const DpRange& r) -> int { return bf_dp_fix_launch(c, st, dopt, r); };
    // dhd: dA1 = ([dA2 | dA6] [W2 | W6]^T) (1 - hd^2)  and  dW2 (| dW6) = hd^T [dA2 | dA6] ->
    // optimizer: both need only the decoder's outputs; unforked (DP, profiling, VAEB_BF_FORK=0)
    // they share one grid of 256 x 256 tiles (bf_gemm2)
    const bf::EpiDTanh e_dhd = h16_guarded(c, bf::EpiDTanh{b.hd, H, LM, H, b.dA1, H, b.cp1});
    bf::Opt o26 = opt;
    o26.shadow_out = b.shadow2[par ^ 1] + b.s26;
    bf::EpiAdagrad e_w26{cmap(gs ? 2 : 0, 0, c->off[sl.W2], gs ? c->off[sl.W6] : 0, D, D), o26, H, Dn};
    e_w26.vec = adagrad_vec(e_w26);
    // fork (not profiled, not DP): dhd on the whole chip first; then the weight gradients
    // off the critical path -- dW1, dW2 (| dW6) on 128 256 x 256 tiles, and (once [dMu | dLv]
    // is ready) dW4 | dW5 -- run on the second stream beside the chain dz -> [dMu | dLv] ->
    // dh -> dW3 that the step's end waits for; joined at the step's end
    // DP (round 3): the same fork; the forked weight gradients store their data gradients,
    // bucket A (W2 | W6) is all-reduced and updated on s3 right after dW2, and the rest is
    // reduced on s once s3 has joined (world-1 DP step 923 -> see DESIGN.md 5)
    const bool fork = c->bf_fork && !prof && c->s3;
    // dz fused into the forked dhd (transposed, on 8-phase 256 x 256 tiles): Z <= 128, Z % 16 == 0
    const bool dzf = fork && c->bf_dzfuse && c->bf_dtt && H % 8 == 0 && Z <= 128 && Z % 16 == 0 && use8<bf::KC, bf::KC>();
    const hipStream_t sw = fork ? c->s3 : s;   // the off-path weight gradients' stream
    if (fork) {
        pr.mark(K_BF_DHD);
        if (dzf) {
            // ... and dZ as split-K slabs from the dA1 tile in LDS (EpiDTanhTDz, VAEB_BF_DZFUSE)
            const bf::EpiDTanhTDz e =
                h16_guarded(c, bf::EpiDTanhTDz{{b.hd, H, LM, H, b.dA1, H, b.cp1}, sh + b.s1, Z, H, b.dz_slab, (int64_t)LM * Z});
            const bf::GemmArgs g1 = bf_args256(sh + b.s26, Dn, (int64_t)H * Dn * 2, b.dA, Dn, (int64_t)LM * Dn * 2, H, LM, Dn);
            REP(pr) if (int rc = bf_launch8<bf::KC, bf::KC>(s, g1, 1, e)) return rc;
        } else if (c->bf_dtt && H % 8 == 0) {
            // the transposed product dA1^T = W2 dA^T (EpiDTanhT: 8-byte LDS epilogue accesses)
            const bf::EpiDTanhT e = h16_guarded(c, bf::EpiDTanhT{b.hd, H, LM, H, b.dA1, H, b.cp1});
            REP(pr) if (int rc = bf_gemm<bf::KC, bf::KC>(s, sh + b.s26, Dn, (int64_t)H * Dn * 2, b.dA, Dn,
                                                          (int64_t)LM * Dn * 2, H, LM, Dn, 1, e)) return rc;
        } else {
            REP(pr) if (int rc = bf_gemm<bf::KC, bf::KC>(s, b.dA, Dn, (int64_t)LM * Dn * 2, sh + b.s26, Dn,
                                                          (int64_t)H * Dn * 2, LM, H, Dn, 1, e_dhd)) return rc;
        }
    } else {
        const bf::GemmArgs gw = bf_args256(b.hd, H, (int64_t)LM * H * 2, b.dA, Dn, (int64_t)LM * Dn * 2, H, Dn, LM);
        const bf::GemmArgs gd = bf_args256(b.dA, Dn, (int64_t)LM * Dn * 2, sh + b.s26, Dn, (int64_t)H * Dn * 2, LM, H, Dn);
        pr.mark(K_BF_DHD_DW26);
        REP(pr) if (int rc = bf_gemm2<bf::KO, bf::KO, bf::EpiAdagrad, bf::KC, bf::KC, bf::EpiDTanh>(s, gw, e_w26, gd, e_dhd))
            return rc;
    }
    if (dp && !fork) if (int rc = dp_bucket_a(c, pr, dopt.th_out, dp_opt, dp_fix)) return rc;
    // dz slabs = dA1 W1^T  (thin: dz + latent backward in one launch, after dW1's fork below)
    const int ksz = bf_slices(H, b.ks_dz);
    if (!b.thin_z && !dzf) pr.mark(K_BF_DZ);
    if (!b.thin_z && !dzf)
    REP(pr) if (int rc = bf_gemm<bf::KC, bf::KC>(s, b.dA1, H, (int64_t)LM * H * 2, sh + b.s1, H, (int64_t)Z * H * 2,
                                                  LM, Z, H, b.ks_dz,
                                                  bf::EpiF32{b.dz_slab, Z, LM, Z, (int64_t)LM * Z})) return rc;
    // The second stream's launches (the round-4 order, ELBO_FIRST / W1_FIRST builds removed: the
    // forked dW2 (| dW6) first, so the long product starts earliest, then dW1 (+ its optimizer)
    // and the ELBO's stage-1 partials, which need only the decoder's log p and the latent terms
    // (bias_opt's last block waits for them).  Unforked: dW1 in place on s.
    const bf::GemmArgs gw2 = bf_args256(b.hd, H, (int64_t)LM * H * 2, b.dA, Dn, (int64_t)LM * Dn * 2, H, Dn, LM);
    // (round 5 measured and removed: only the first a of dW2's column tiles forked, the rest in
    // one grid with dW3 after dh -- a = 12 +2-4 us, 8 +10-13, 4 +35 us per step)
    auto side = [&]() -> int {
        if (fork) {
            if (int rc = bf_wgrad256(c->s3, gw2, e_w26)) return rc;
            if (dp && c->dp_overlap) {
                // bucket A right behind its gradient, on the fork's stream: reduced (dp_ev[1]) and
                // updated (dp_ev[2]) beside the dz -> dh -> dW3 chain
                if (int rc = dp_reduce_update(c, c->s3, dp_bucket_a_runs(c), dopt.th_out, dp_opt, dp_fix, c->dp_ev[1]))
                    return rc;
                HIP_TRY(hipEventRecord(c->dp_ev[2], c->s3));
            }
        }
        // dW1 = z^T dA1 (split-K slabs) -> optimizer
        const int ks1 = bf_slices(LM, b.ks_w1);
        pr.mark(K_BF_DW1);
        REP(pr) if (int rc = bf_gemm<bf::KO, bf::KO>(sw, b.z, Z, (int64_t)LM * Z * 2, b.dA1, H, (int64_t)LM * H * 2,
                                                      Z, H, LM, b.ks_w1,
                                                      bf::EpiF32{b.w_slab, H, Z, H, (int64_t)Z * H})) return rc;
        bf::WReduceArgs w{};
        w.slab = b.w_slab; w.nslab = ks1; w.M = Z; w.N = H;
        w.map = cmap(0, 0, c->off[sl.W1], 0, H, 0);
        w.opt = opt; w.opt.shadow_out = b.shadow2[par ^ 1] + b.s1;
        pr.mark(K_BF_DW1_OPT);
        REP(pr) hipLaunchKernelGGL(bf::wreduce_opt_kernel, dim3(std::min(1024, cdiv((int64_t)Z * H, 256))), dim3(256),
                                   0, sw, w);
        CHECK_LAUNCH();
        return 0;
    };
    // The second stream forks off right after dhd: dz and dh share the chip with dW2.  (Round 5
    // measured the other fork points and removed them: after dz + [dMu | dLv] +3-5 us per step,
    // after dh +35-40 us, the main chain captured first +13-17 us then.)
    if (fork) {
        HIP_TRY(hipEventRecord(c->fk_ev[0], s));
        HIP_TRY(hipStreamWaitEvent(c->s3, c->fk_ev[0], 0));
    }
    if (int rc = side()) return rc;
    // [dMu | dLv]
    bf::LatentArgs la{};
    la.M = M; la.Z = Z; la.L = L; la.est = g.estimator; la.mode = MODE_TRAIN;
    // (the latent backward's KL / LA terms join the loss-scaled dZ: h16_scale)
    la.sc = ((g.objective == VAEB_OBJ_MEAN_MAP) ? 1.0f / (float)g.B_global : 1.0f) * h16_scale(c);
    la.mu = b.mu; la.lv = b.lv; la.eps = b.eps;
    la.dz_slab = b.dz_slab; la.ndz = ksz; la.dmulv = b.dml; la.colpart = b.cp45;
    la = h16_guarded(c, la);
    pr.mark(K_BF_LATENT_BWD);
    if (dzf) {
        // the dhd blocks stored dZ as cdiv(H, 256) split-K slabs: the latent backward sums them
        la.ndz = cdiv(H, 256);
        if (bf_lat4(c, la))
            REP(pr) hipLaunchKernelGGL(bf::latent_bwd_v4_kernel, dim3(cdiv(M, bf::kLbRows), cdiv(Z, 128)), dim3(256), 0, s, la);
        else
            REP(pr) hipLaunchKernelGGL(bf::latent_bwd_kernel, dim3(cdiv(M, bf::kLbRows), cdiv(2 * Z, 64)), dim3(256), 0, s, la);
    } else if (b.thin_z) {
        bf::ThinArgs ta{};
        ta.A = b.dA1; ta.lda = H; ta.a_bytes = (int64_t)LM * H * 2; ta.M = M;
        ta.B = sh + b.s1; ta.ldb = H; ta.b_bytes = (int64_t)Z * H * 2; ta.K = H; ta.bcol1 = -1;
        bf::EpiDzLatent ez{};
        ez.mu = b.mu; ez.lv = b.lv; ez.eps = b.eps; ez.dmulv = b.dml; ez.colpart = b.cp45;
        ez.sc = la.sc; ez.M = M; ez.Z = Z;
        REP(pr) if (int rc = bf_thin<bf::KC, 32>(s, ta, dim3(cdiv(M, 32), Z / 128), h16_guarded(c, ez))) return rc;
    } else if (bf_lat4(c, la))
        REP(pr) hipLaunchKernelGGL(bf::latent_bwd_v4_kernel, dim3(cdiv(M, bf::kLbRows), cdiv(Z, 128)), dim3(256), 0, s, la);
    else
        REP(pr) hipLaunchKernelGGL(bf::latent_bwd_kernel, dim3(cdiv(M, bf::kLbRows), cdiv(2 * Z, 64)), dim3(256), 0, s, la);
    CHECK_LAUNCH();
    if (fork) {
        HIP_TRY(hipEventRecord(c->fk_ev[2], s));
        HIP_TRY(hipStreamWaitEvent(c->s3, c->fk_ev[2], 0));
    }
    // dh: dA3 = ([dMu | dLv] [W4 | W5]^T) (1 - h^2)
    pr.mark(K_BF_DH);
    if (c->bf_dtt && H % 8 == 0) {
        // the transposed product dA3^T = [W4 | W5] [dMu | dLv]^T (EpiDTanhT)
        REP(pr) if (int rc = bf_gemm<bf::KC, bf::KC>(s, sh + b.s45, 2 * Z, (int64_t)H * 2 * Z * 2, b.dml, 2 * Z,
                                                      (int64_t)M * 2 * Z * 2, H, M, 2 * Z, 1,
                                                      h16_guarded(c, bf::EpiDTanhT{b.h, H, M, H, b.dA3, H, b.cp3}))) return rc;
    } else {
        REP(pr) if (int rc = bf_gemm<bf::KC, bf::KC>(s, b.dml, 2 * Z, (int64_t)M * 2 * Z * 2, sh + b.s45, 2 * Z,
                                                      (int64_t)H * 2 * Z * 2, M, H, 2 * Z, 1,
                                                      h16_guarded(c, bf::EpiDTanh{b.h, H, M, H, b.dA3, H, b.cp3}))) return rc;
    }
    // dW4 | dW5 = h^T [dMu | dLv] (split-K slabs) -> optimizer
    {
        const int ks45 = bf_slices(M, b.ks_w45);
        pr.mark(K_BF_DW45);
        REP(pr) if (int rc = bf_gemm<bf::KO, bf::KO>(sw, b.h, H, (int64_t)M * H * 2, b.dml, 2 * Z, (int64_t)M * 2 * Z * 2,
                                                      H, 2 * Z, M, b.ks_w45,
                                                      bf::EpiF32{b.w_slab, 2 * Z, H, 2 * Z, (int64_t)H * 2 * Z})) return rc;
        bf::WReduceArgs w{};
        w.slab = b.w_slab; w.nslab = ks45; w.M = H; w.N = 2 * Z;
        w.map = cmap(1, Z, c->off[sl.W4], c->off[sl.W5], Z, Z);
        w.opt = opt; w.opt.shadow_out = b.shadow2[par ^ 1] + b.s45;
        pr.mark(K_BF_DW45_OPT);
        REP(pr) hipLaunchKernelGGL(bf::wreduce_opt_kernel, dim3(std::min(1024, cdiv((int64_t)H * 2 * Z, 256))),
                                   dim3(256), 0, sw, w);
        CHECK_LAUNCH();
    }
    // dW3 = X^T dA3 -> optimizer
    {
        bf::Opt o = opt;
        o.shadow_out = b.shadow2[par ^ 1] + b.s3;
        bf::EpiAdagrad e{cmap(0, 0, c->off[sl.W3], 0, H, 0), o, D, H};
        e.vec = adagrad_vec(e);
        pr.mark(K_BF_DW3);
        if (fork) {
            // beside the forked dW2 (128 256 x 256 tiles) each product holds half the chip:
            // 256 x 256 tiles here too (ping-pong, the better tile) instead of 256 x 128
            // tiles that the forked dW2's long tiles would leave one round trip of CUs
            const bf::GemmArgs g3 = bf_args256(x0, D, (int64_t)M * D * 2, b.dA3, H, (int64_t)M * H * 2, D, H, M, 1, xb);
            if (int rc = bf_wgrad256(s, g3, e)) return rc;
        } else {
            REP(pr) if (int rc = bf_gemm<bf::KO, bf::KO>(s, x0, D, (int64_t)M * D * 2, b.dA3, H, (int64_t)M * H * 2,
                                                          D, H, M, 1, e, xb)) return rc;
        }
    }
    // biases + ELBO
    {
        bf::BiasArgs ba{};
        const int nrbM = bf_rowblocks(M), nrbL = bf_rowblocks(LM);
        // (the transposed dh / dhd epilogues number their column-partial rows per their tiles)
        const bool dtt = c->bf_dtt && H % 8 == 0;
        const int nrb3 = dtt ? bf_rowblocks_t(M, H) : nrbM;
        const int nrb1 = dzf ? cdiv(LM, 256) * 4 : (fork && dtt) ? bf_rowblocks_t(LM, H) : nrbL;
        ba.seg[0] = bf::BiasSeg{b.cp3, nrb3, H, cmap(0, 0, c->off[sl.b3], 0, 0, 0)};
        ba.seg[1] = bf::BiasSeg{b.cp45, cdiv(M, bf::kLbRows), 2 * Z, cmap(1, Z, c->off[sl.b4], c->off[sl.b5], 0, 0)};
        ba.seg[2] = bf::BiasSeg{b.cp1, nrb1, H, cmap(0, 0, c->off[sl.b1], 0, 0, 0)};
        ba.seg[3] = bf::BiasSeg{b.cp26, nrbL, Dn, cmap(gs ? 2 : 0, 0, c->off[sl.b2], gs ? c->off[sl.b6] : 0, 0, 0)};
        ba.nseg = 4;
        ba.total = H + 2 * Z + H + Dn;
        int nbias = 0;
        for (int k = 0; k < 4; ++k) nbias += (ba.segblk[k] = cdiv(ba.seg[k].N, 64));
        ba.opt = opt;
        ElboArgs e = bf_elbo(c, M);
        e.elbo_out = c->elbo_out; e.epoch = c->epoch; e.cursor = cursor; e.step = c->step;
        if (dp) { e.dp_slot = c->grad + c->P; e.elbo_out = nullptr; e.cursor = nullptr; e.step = nullptr; }
        ba.elbo = e;
        ba.elbo_parts = b.elbo_parts; ba.n_elbo_parts = bf::kElboBlocks;
        pr.mark(K_BF_BIAS_ELBO);
        if (fork) {
            // the ELBO's stage-1 partials on the main stream after dW3: the second stream's tail,
            // not the main chain, ends the step once dz is in dhd (round 5: -2 us against them on
            // the second stream)
            hipLaunchKernelGGL(bf::elbo_partial_kernel, dim3(bf::kElboBlocks), dim3(256), 0, s, bf_elbo(c, M), b.elbo_parts);
            hipLaunchKernelGGL(bf::bias_opt_kernel, dim3(nbias + 1), dim3(256), 0, s, ba);
        } else {
            REP(pr) {
                hipLaunchKernelGGL(bf::elbo_partial_kernel, dim3(bf::kElboBlocks), dim3(256), 0, s, e, b.elbo_parts);
                hipLaunchKernelGGL(bf::bias_opt_kernel, dim3(nbias + 1), dim3(256), 0, s, ba);
            }
        }
        CHECK_LAUNCH();
        if (fork && dp) {
            // the forked gradients (dW1, dW45 and, without overlap, dW2 | dW6) are bucket B's:
            // join before reducing it
            HIP_TRY(hipEventRecord(c->fk_ev[1], c->s3));
            HIP_TRY(hipStreamWaitEvent(s, c->fk_ev[1], 0));
        }
        if (dp) if (int rc = dp_bucket_b(c, pr, K_BF_ADAGRAD_DP, dopt.th_out, dp_opt, dp_fix)) return rc;
    }
    if (fork && !dp) {
        HIP_TRY(hipEventRecord(c->fk_ev[1], c->s3));
        HIP_TRY(hipStreamWaitEvent(s, c->fk_ev[1], 0));
    }
    pr.mark(K_END);
    c->prof_n = pr.k;
    return 0;
}

// validate / reconstruct for the bf16 engine: one device chunk of bf16 rows x (global
// rows [r0, r0 + rows) for the noise keys and the host eps rows).
int bf_eval_chunk_dev(vaeb_ctx* c, const bf16_t* x, int rows, int64_t r0, int mode, float* out_y) {
    const vaeb_config& g = c->c;
    bf::BfState& b = c->bf;
    BfFwd f{};
    f.Mb = rows; f.mode = mode; f.train = false; f.x = x; f.xb = bf::BatchRef{};
    f.row_base_mul = 0; f.row_base_add = r0;
    f.eps_in = c->eps_in ? c->eps_in + r0 * g.Z : nullptr; f.eps_in_ld = c->eps_rows; f.domain = 1;
    f.yout = (mode == MODE_RECON) ? c->y : nullptr;
    Prof pr{c, false};
    if (int rc = bf_forward(c, c->par, f, pr)) return rc;
    if (mode == MODE_RECON) {
        HIP_TRY(hipMemcpyAsync(out_y, c->y, sizeof(float) * (size_t)rows * g.D, hipMemcpyDeviceToHost, c->s));
    } else {
        ElboArgs e = bf_elbo(c, rows);
        e.eval_acc = c->eval_acc;
        hipLaunchKernelGGL(bf::elbo_partial_kernel, dim3(bf::kElboBlocks), dim3(256), 0, c->s, e, b.elbo_parts);
        hipLaunchKernelGGL(bf::elbo_final_kernel, dim3(1), dim3(256), 0, c->s, e, (const double*)b.elbo_parts,
                           bf::kElboBlocks);
        CHECK_LAUNCH();
    }
    return 0;
}

// ... of host fp32 rows (uploaded through the eval staging buffers).
int bf_eval_chunk(vaeb_ctx* c, const float* x, int rows, int64_t r0, int mode, float* out_y) {
    if (int rc = bf_upload_rows(c, x, rows, c->bf.xeval)) return rc;
    return bf_eval_chunk_dev(c, c->bf.xeval, rows, r0, mode, out_y);
}

// ---------------------------------------------------------------- GEMM test / bench hooks
// (vaeb_test_gemm_bf16 / vaeb_bench_gemm_bf16 of include/vaeb_diag.h, on the context's 16-bit type)
int h16_test_gemm(vaeb_ctx* c, int32_t ako, int32_t bko, int32_t M, int32_t N, int32_t K, const float* A,
                        const float* B, float* C, int32_t ksplit) {
    // ksplit < 0: the 256 x 256 8-phase main loop (gemm8_kernel) with -ksplit slices;
    // -22: two slices combined in the launch (split2_combine), one output
    const bool split2 = ksplit == -22;
    if (split2) ksplit = -2;
    const bool force8 = ksplit < 0;
    if (force8) ksplit = -ksplit;
    if (!c || !A || !B || !C || M <= 0 || N <= 0 || K <= 0 || ksplit <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (K % 8 || (ako && M % 8) || (bko && N % 8))
        return fail(VAEB_ERR_ARG, "bf16 GEMM: K (and a K-outer operand's rows) must be multiples of 8");
    const size_t na = (size_t)M * K, nb = (size_t)N * K;
    const int nz = bf_slices(K, ksplit);
    float *fa = nullptr, *fb = nullptr, *fc = nullptr;
    bf16_t *ba = nullptr, *bb = nullptr;
    int rc = 0;
    rc = rc ? rc : dalloc(&fa, na);
    rc = rc ? rc : dalloc(&fb, nb);
    rc = rc ? rc : dalloc(&ba, na);
    rc = rc ? rc : dalloc(&bb, nb);
    rc = rc ? rc : dalloc(&fc, (size_t)nz * M * N);
    float* part = nullptr;
    int* ticket = nullptr;
    const int tiles256 = cdiv(M, bf::BM) * cdiv(N, 256);
    if (split2) {
        rc = rc ? rc : dalloc(&part, (size_t)tiles256 * 65536);
        rc = rc ? rc : dalloc(&ticket, (size_t)tiles256);
    }
    if (!rc) {
        hipMemcpy(fa, A, na * 4, hipMemcpyHostToDevice);
        hipMemcpy(fb, B, nb * 4, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(bf::to_bf16_kernel, dim3(256), dim3(256), 0, c->s, fa, ba, (int64_t)na);
        hipLaunchKernelGGL(bf::to_bf16_kernel, dim3(256), dim3(256), 0, c->s, fb, bb, (int64_t)nb);
        const bf::EpiF32 e{fc, N, M, N, (int64_t)M * N};
        const int lda = ako ? M : K, ldb = bko ? N : K;
        const int64_t ab = (int64_t)na * 2, bbytes = (int64_t)nb * 2;
        if (force8) {
            bf::GemmArgs g = bf_args256(ba, lda, ab, bb, ldb, bbytes, M, N, K, ksplit);
            if (split2) {
                g.part = part;
                g.ticket = ticket;
                g.kslice = ((cdiv(K, 2) + 63) / 64) * 64;
            }
            if (!ako && !bko) rc = bf_launch8<bf::KC, bf::KC>(c->s, g, nz, e);
            else if (!ako && bko) rc = bf_launch8<bf::KC, bf::KO>(c->s, g, nz, e);
            else if (ako && !bko) rc = bf_launch8<bf::KO, bf::KC>(c->s, g, nz, e);
            else rc = bf_launch8<bf::KO, bf::KO>(c->s, g, nz, e);
        } else if (!ako && !bko) rc = bf_gemm<bf::KC, bf::KC>(c->s, ba, lda, ab, bb, ldb, bbytes, M, N, K, ksplit, e);
        else if (!ako && bko) rc = bf_gemm<bf::KC, bf::KO>(c->s, ba, lda, ab, bb, ldb, bbytes, M, N, K, ksplit, e);
        else if (ako && !bko) rc = bf_gemm<bf::KO, bf::KC>(c->s, ba, lda, ab, bb, ldb, bbytes, M, N, K, ksplit, e);
        else rc = bf_gemm<bf::KO, bf::KO>(c->s, ba, lda, ab, bb, ldb, bbytes, M, N, K, ksplit, e);
    }
    if (!rc) {
        std::vector<float> slabs((size_t)nz * M * N);
        hipError_t e = hipStreamSynchronize(c->s);
        if (e == hipSuccess) e = hipMemcpy(slabs.data(), fc, slabs.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(VAEB_ERR_HIP, "test gemm: %s", hipGetErrorString(e));
        for (size_t i = 0; !rc && i < (size_t)M * N; ++i) {
            float v = 0.f;
            for (int z = 0; z < nz; ++z) v += slabs[(size_t)z * M * N + i];
            C[i] = v;
        }
    }
    if (!rc && split2) {   // every ticket back at zero
        std::vector<int> tk(tiles256);
        if (hipMemcpy(tk.data(), ticket, tk.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(VAEB_ERR_HIP, "test gemm: ticket copy");
        for (int t : tk) if (!rc && t != 0) rc = fail(VAEB_ERR_HIP, "test gemm: split-K ticket left at %d", t);
    }
    for (void* p : {(void*)fa, (void*)fb, (void*)fc, (void*)ba, (void*)bb, (void*)part, (void*)ticket}) if (p) hipFree(p);
    return rc;
}

// Diagnostics: device-side uniform [-1, 1) 16-bit fill (a hash of the index), no host copy.
__global__ __launch_bounds__(256) void fill_bf16_kernel(bf16_t* p, int64_t n, uint32_t seed) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        uint32_t h = (uint32_t)i * 0x9E3779B1u ^ seed;
        h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
        p[i] = (bf16_t)bf::f2bf((float)(h >> 8) * (2.0f / 16777216.0f) - 1.0f);
    }
}

template <int LA, int LB>
int bench_gemm_launch(hipStream_t s, const bf16_t* A, const bf16_t* B, int M, int N, int K, int bn,
                             const bf::EpiBiasAct& e, float* part, int* ticket) {
    bf::GemmArgs g{};
    g.A = A; g.lda = LA == bf::KO ? M : K; g.a_bytes = (int64_t)M * K * 2;
    g.B = B; g.ldb = LB == bf::KO ? N : K; g.b_bytes = (int64_t)N * K * 2;
    g.M = M; g.N = N; g.K = K;
    g.tiles_m = cdiv(M, bf::BM); g.tiles_n = cdiv(N, bn);
    g.kslice = ((K + bf::BK - 1) / bf::BK) * bf::BK;
    if (bn == 8 || bn == 9) {
        g.tiles_n = cdiv(N, 256);
        if (bn == 9) {   // two K slices combined in the launch (split2_combine)
            g.part = part;
            g.ticket = ticket;
            g.kslice = ((cdiv(K, 2) + 63) / 64) * 64;
        }
        return bf_launch8<LA, LB>(s, g, bn == 9 ? 2 : 1, e);
    }
    if (bn == 256) return bf_launch<LA, LB, 256>(s, g, 1, e);
    return bf_launch<LA, LB, 128>(s, g, 1, e);
}

int h16_bench_gemm(vaeb_ctx* c, int32_t ako, int32_t bko, int32_t M, int32_t N, int32_t K, int32_t bn,
                         int32_t reps, float* out_ms) {
    if (!c || !out_ms || M <= 0 || N <= 0 || K <= 0 || reps <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (K % 8 || M % 8 || N % 8) return fail(VAEB_ERR_ARG, "bench gemm: M, N, K must be multiples of 8");
    if (bn == 0) bn = bf_bn(M, N);
    if (bn != 128 && bn != 256 && bn != 8 && bn != 9)
        return fail(VAEB_ERR_ARG, "bench gemm: tile width 128 or 256 (8: 256 x 256 on the 8-phase loop, "
                                  "9: the same as two K slices)");
    bf16_t *a = nullptr, *b = nullptr, *o = nullptr;
    float *bias = nullptr, *part = nullptr;
    int* ticket = nullptr;
    int rc = 0;
    if (bn == 9) {
        const int tiles = cdiv(M, bf::BM) * cdiv(N, 256);
        rc = rc ? rc : dalloc(&part, (size_t)tiles * 65536);
        rc = rc ? rc : dalloc(&ticket, (size_t)tiles);
    }
    rc = rc ? rc : dalloc(&a, (size_t)M * K);
    rc = rc ? rc : dalloc(&b, (size_t)N * K);
    rc = rc ? rc : dalloc(&o, (size_t)M * N);
    rc = rc ? rc : dalloc(&bias, (size_t)N);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!rc) {
        hipLaunchKernelGGL(fill_bf16_kernel, dim3(1024), dim3(256), 0, c->s, a, (int64_t)M * K, 1u);
        hipLaunchKernelGGL(fill_bf16_kernel, dim3(1024), dim3(256), 0, c->s, b, (int64_t)N * K, 2u);
        const bf::EpiBiasAct e{bias, 0, M, N, o, N};
        auto one = [&]() {
            if (!ako && !bko) return bench_gemm_launch<bf::KC, bf::KC>(c->s, a, b, M, N, K, bn, e, part, ticket);
            if (!ako && bko) return bench_gemm_launch<bf::KC, bf::KO>(c->s, a, b, M, N, K, bn, e, part, ticket);
            if (ako && !bko) return bench_gemm_launch<bf::KO, bf::KC>(c->s, a, b, M, N, K, bn, e, part, ticket);
            return bench_gemm_launch<bf::KO, bf::KO>(c->s, a, b, M, N, K, bn, e, part, ticket);
        };
        rc = one();   // warm-up
        hipEventCreate(&e0);
        hipEventCreate(&e1);
        hipEventRecord(e0, c->s);
        for (int r = 0; !rc && r < reps; ++r) rc = one();
        hipEventRecord(e1, c->s);
        if (!rc && hipEventSynchronize(e1) == hipSuccess) {
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            *out_ms = ms / (float)reps;
        }
    }
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    for (void* p : {(void*)a, (void*)b, (void*)o, (void*)bias, (void*)part, (void*)ticket}) if (p) hipFree(p);
    return rc;
}

// vaeb_dp_rank_update (diagnostics): this rank's optimizer launch over `own` and the shadow fix
// over `fr`, the step's own launches (bf_dp_opt_launch / bf_dp_fix_launch) on the context stream
int h16_dp_opt(vaeb_ctx* c, int par, const DpRange& own) { return bf_dp_opt_launch(c, c->s, bf_opt(c, par, true, false), own, ElboArgs{}); }
int h16_dp_fix(vaeb_ctx* c, int par, const DpRange& fr) { return bf_dp_fix_launch(c, c->s, bf_opt(c, par, true, false), fr); }
