// engine_bf16.inc -- host orchestration of the 16-bit large-batch step (step_bf16.hpp).
// Included by vaeb_hip.hip inside its anonymous namespace, after the fp32 helpers, twice:
// namespace eng_bf (bf = vaeb::bf, bf16 operands) and eng_hf (bf = vaeb::hf, fp16 operands), kF16
// telling them apart (h16_engines.hpp).  vaeb_create admits a 16-bit context only with D, H and Z
// multiples of 8; nothing here tests that again.
//
// Call map (one launch site per kernel family; DESIGN.md 4.2 "Host structure"):
//   operands      mat() is the one place a byte extent is computed; bf_mats() the step's views;
//                 gemm_args() / thin_args() the one fill of GemmArgs / ThinArgs
//   launches      bf_launch_lds (> 64 KiB LDS: attribute once per kernel instantiation, launch, check)
//                 <- bf_launch8 | bf_launch | bf_thin | bf_gemm2;  bf_gemm / bf_gemm_2b pick the tile
//   bf_forward    enc | heads (thin: + latent) | latent | dechid | decout       (training and evaluation)
//   bf_train_step bf_step_form -> bf_forward -> dhd (| dW26 in its grid) -> dz -> [fork: dW26] dW1
//                 (bf_wgrad_slabs) -> bf_latent_bwd | thin dz -> dh -> dW45 (bf_wgrad_slabs) -> dW3 ->
//                 bias + ELBO, its partial rows from bf_partial_rows of the forms the plan recorded
//   evaluation    eval_chunks (vaeb_hip.hip: stages host rows with bf_upload_rows) -> bf_eval_chunk_dev ->
//                 bf_forward on bf_eval_fwd (vaeb_hip.hip)
//   memory        BfState::mem (dev_owner.hpp) owns every buffer: bf_alloc's, and the dataset copies
//                 x, xbits and xval that vaeb_set_data / vaeb_set_valid_data replace; bf_free releases it

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
// The objective's scale of every data term: 1 / B_global for the mean objective.
float bf_obj_scale(const vaeb_ctx* c) { return c->c.objective == VAEB_OBJ_MEAN_MAP ? 1.0f / (float)c->c.B_global : 1.0f; }

// fp16: the guard word that a training step's range-checked 16-bit stores report to
// (h16_engines.hpp, H16_GUARD_FIELD); the bf16 structs have no such member.
template <class E>
E h16_guarded(vaeb_ctx* c, E e, bool train = true) {
    if constexpr (kF16) {
        if (train) e.guard = c->blk + kBlkFxErr;
    }
    return e;
}

// ---------------------------------------------------------------- operand views
// A 16-bit matrix as the kernels' buffer descriptors see it: rows of ld elements from p, `bytes`
// readable.  mat() is the only place the extent is computed.
struct Mat { const bf16_t* p; int ld; int64_t bytes; };
Mat mat(const bf16_t* p, int64_t rows, int ld) { return Mat{p, ld, rows * ld * 2}; }

// The step's operands for M rows of x (LM = L * M sample rows) and the shadow weights of arena par.
struct BfMats { Mat X, h, z, hd, dA, dA1, dml, dA3, W3, W45, W1, W26; };
BfMats bf_mats(const vaeb_ctx* c, int par, const bf16_t* x, int M) {
    const bf::BfState& b = c->bf;
    const int D = c->c.D, H = c->c.H, Z = c->c.Z, Dn = b.Dn;
    const int64_t LM = (int64_t)c->c.L * M;
    const bf16_t* sh = b.shadow2[par];
    return BfMats{mat(x, M, D), mat(b.h, M, H), mat(b.z, LM, Z), mat(b.hd, LM, H), mat(b.dA, LM, Dn), mat(b.dA1, LM, H),
                  mat(b.dml, M, 2 * Z), mat(b.dA3, M, H),
                  mat(sh + b.s3, D, H), mat(sh + b.s45, H, 2 * Z), mat(sh + b.s1, Z, H), mat(sh + b.s26, H, Dn)};
}

// K per split-K slice (a multiple of BK) and the slices that leaves.
int bf_kslice(int K, int slices) { return cdiv(cdiv(K, std::max(1, slices)), bf::BK) * bf::BK; }
int bf_slices(int K, int ks) { return cdiv(K, bf_kslice(K, ks)); }

// GemmArgs of A B on 256 x tile_n tiles, K in `slices` slices.
bf::GemmArgs gemm_args(const Mat& A, const Mat& B, int M, int N, int K, int tile_n, int slices = 1,
                       bf::BatchRef ab = bf::BatchRef{}) {
    bf::GemmArgs g{};
    g.A = A.p; g.lda = A.ld; g.a_bytes = A.bytes; g.ab = ab;
    g.B = B.p; g.ldb = B.ld; g.b_bytes = B.bytes;
    g.M = M; g.N = N; g.K = K;
    g.tiles_m = cdiv(M, bf::BM); g.tiles_n = cdiv(N, tile_n);
    g.kslice = bf_kslice(K, slices);
    return g;
}
bf::ThinArgs thin_args(const Mat& A, int M, const Mat& B, int K, int bcol1) {
    bf::ThinArgs t{};
    t.A = A.p; t.lda = A.ld; t.a_bytes = A.bytes; t.M = M;
    t.B = B.p; t.ldb = B.ld; t.b_bytes = B.bytes; t.K = K; t.bcol1 = bcol1;
    return t;
}

// ---------------------------------------------------------------- launches
// Block-tile width for an M x N product: 256-wide tiles unless that leaves the chip
// (256 CUs, one block each) less than full.
int bf_bn(int M, int N) { return cdiv(M, bf::BM) * cdiv(N, 256) >= 256 ? 256 : 128; }

// The launch of a kernel with > 64 KiB of dynamic LDS: its attribute is set once per process per
// kernel instantiation (Kern is a template argument, so the flag is that instantiation's own).
template <auto Kern, class... A>
int bf_launch_lds(dim3 grid, int lds, hipStream_t s, const A&... a) {
    static bool attr_set = false;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_set = true;
    }
    hipLaunchKernelGGL(Kern, grid, dim3(bf::NTHR), lds, s, a...);
    CHECK_LAUNCH();
    return 0;
}

template <int LA, int LB, class E>
int bf_launch8(hipStream_t s, const bf::GemmArgs& g, int nz, const E& e) {
    return bf_launch_lds<bf::gemm8_kernel<LA, LB, E>>(dim3(g.tiles_m * g.tiles_n, nz), bf::lds8_bytes(), s, g, e);
}

template <int LA, int LB, int BNT, class E, int ST = 4>
int bf_launch(hipStream_t s, const bf::GemmArgs& g, int nz, const E& e) {
    // (the Gaussian decoder's epilogue pairs fragment tiles 32 columns apart: gemm_body only)
    if constexpr (BNT == 256 && ST == 4 && !std::is_same_v<E, bf::EpiDecOut<true>>) {
        if (use8<LA, LB>()) return bf_launch8<LA, LB, E>(s, g, nz, e);
    }
    return bf_launch_lds<bf::gemm_kernel<LA, LB, BNT, E, ST>>(dim3(g.tiles_m * g.tiles_n, nz), bf::lds_bytes<BNT, ST>(), s, g, e);
}

// thin_bf16.hpp launches
template <int LB, int BMT, class E>
int bf_thin(hipStream_t s, const bf::ThinArgs& t, dim3 grid, const E& e) {
    return bf_launch_lds<bf::thin_kernel<LB, BMT, E>>(grid, bf::ThinShape<BMT>::kSmem, s, t, e);
}

// A B on the tile width bf_bn picks, K in ks split-K slices (one grid row each).
template <int LA, int LB, class E>
int bf_gemm(hipStream_t s, const Mat& A, const Mat& B, int M, int N, int K, int ks, const E& e,
            bf::BatchRef ab = bf::BatchRef{}) {
    const int bn = bf_bn(M, N);
    const bf::GemmArgs g = gemm_args(A, B, M, N, K, bn, ks, ab);
    const int nz = cdiv(K, g.kslice);
    if (bn == 256) return bf_launch<LA, LB, 256>(s, g, nz, e);
    return bf_launch<LA, LB, 128>(s, g, nz, e);
}

// Two products in one 256 x 256-tile grid (gemm2_kernel): product 1's blocks first.
template <int LA1, int LB1, class E1, int LA2, int LB2, class E2>
int bf_gemm2(hipStream_t s, const bf::GemmArgs& g1, const E1& e1, const bf::GemmArgs& g2, const E2& e2) {
    const int nb1 = g1.tiles_m * g1.tiles_n, nb2 = g2.tiles_m * g2.tiles_n;
    if (use8<LA1, LB1>() && use8<LA2, LB2>())
        return bf_launch_lds<bf::gemm8x2_kernel<LA1, LB1, E1, LA2, LB2, E2>>(dim3(nb1 + nb2), bf::lds8_bytes(), s, g1, e1,
                                                                            g2, e2, nb1);
    return bf_launch_lds<bf::gemm2_kernel<LA1, LB1, E1, LA2, LB2, E2, 256>>(dim3(nb1 + nb2), bf::lds_bytes<256>(), s, g1, e1,
                                                                          g2, e2, nb1);
}

// A short-K product (dechid K = Z, dh K = 2Z) on 256 x 128 tiles with the 3-stage ring and
// two blocks per CU, so one block's epilogue (activation, tile stores) overlaps the other's
// loads instead of running after them (the 256 x 256 tile does both in series).
template <int LA, int LB, class E>
int bf_gemm_2b(hipStream_t s, const Mat& A, const Mat& B, int M, int N, int K, const E& e) {
    return bf_launch<LA, LB, 128, E, 3>(s, gemm_args(A, B, M, N, K, 128), 1, e);
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

// Split-K slices so that a thin product still puts >= ~256 blocks on the chip, keeping
// >= 4 K tiles per slice.
int bf_split(int M, int N, int K) {
    const int tiles = cdiv(M, bf::BM) * cdiv(N, bf_bn(M, N));
    int ks = cdiv(256, tiles);
    ks = std::min(ks, std::max(1, K / (4 * bf::BK)));
    return std::max(1, ks);
}

// ---------------------------------------------------------------- the step's form
// How a dtanh product (dhd, dh) runs: on A W (EpiDTanh), transposed (EpiDTanhT), or transposed
// with dz fused into it (EpiDTanhTDz).  The form numbers the epilogue's column-partial rows.
enum BfDForm { DF_AW, DF_T, DF_T_DZ };

// Rows of a form's column-partial array for `rows` output rows of `cols` columns.
// DF_AW: one per 64-row wave block of every row tile (the empty ones write zeros).  DF_T: the
// output rows are the product's N' (its M' = cols): four wave slots per 256-row tile (gemm8,
// Col8) or two per 128-row tile (the ring, ColStd).  DF_T_DZ: always gemm8's 256-row tiles.
int bf_partial_rows(BfDForm f, int64_t rows, int cols) {
    switch (f) {
        case DF_T: return bf_bn(cols, (int)rows) == 256 ? cdiv(rows, 256) * 4 : cdiv(rows, 128) * 2;
        case DF_T_DZ: return cdiv(rows, 256) * 4;
        default: return cdiv(rows, bf::BM) * (bf::BM / 64);
    }
}

// One training step's form, decided here and nowhere else.
// fork (not profiled, VAEB_BF_FORK): dhd on the whole chip first; then the weight gradients off
// the critical path -- dW1, dW2 (| dW6) on 128 256 x 256 tiles, and (once [dMu | dLv] is ready)
// dW4 | dW5 -- run on the second stream beside the chain dz -> [dMu | dLv] -> dh -> dW3 that the
// step's end waits for; joined at the step's end.  Unforked, dhd and dW2 (| dW6) share one grid.
// DP (round 3): the same fork; the forked weight gradients store their data gradients, bucket A
// (W2 | W6) is all-reduced and updated on s3 right after dW2, and the rest is reduced on s once
// s3 has joined (world-1 DP step 923 -> see DESIGN.md 5).
struct BfStepForm {
    bool fork;
    bool dtt;             // VAEB_BF_DTT: dhd / dh transposed (EpiDTanhT: 8-byte LDS epilogue accesses)
    bool dzf;             // dz fused into the forked dhd (VAEB_BF_DZFUSE): Z <= 128, Z % 16 == 0, 8-phase tiles
    bool thin_h, thin_z;  // heads + latent / dz + latent backward on the thin launches this step
    hipStream_t sw;       // the off-path weight gradients' stream
    BfDForm dhd, dh;
};
BfStepForm bf_step_form(const vaeb_ctx* c, bool prof) {
    const int Z = c->c.Z;
    BfStepForm p{};
    p.fork = c->bf_fork && !prof && c->s3;
    p.dtt = c->bf_dtt != 0;
    p.dzf = p.fork && c->bf_dzfuse && p.dtt && Z <= 128 && Z % 16 == 0 && use8<bf::KC, bf::KC>();
    p.thin_h = c->bf.thin_h;
    p.thin_z = c->bf.thin_z && !p.dzf;
    p.sw = p.fork ? c->s3 : c->s;
    p.dhd = !p.fork ? DF_AW : p.dzf ? DF_T_DZ : p.dtt ? DF_T : DF_AW;
    p.dh = p.dtt ? DF_T : DF_AW;
    return p;
}

// ---------------------------------------------------------------- memory
int bf_alloc(vaeb_ctx* c) {
    bf::BfState& b = c->bf;
    const vaeb_config& g = c->c;
    const int D = g.D, H = g.H, Z = g.Z, L = g.L;
    const bool gs = gaussian(c);
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
    const int64_t nrbL = bf_partial_rows(DF_AW, RL, H) + 1;
    const bool thin_ok = Z % 128 == 0 && L == 1 && g.estimator == VAEB_EST_LB;
    b.thin_h = thin_ok && (c->bf_thin & 1);
    b.thin_z = thin_ok && (c->bf_thin & 2);
    b.nkl = b.thin_h ? Z / 64 : 1;
    int rc = 0;
    auto own = [&](auto** p, size_t n) { rc = rc ? rc : b.mem.alloc(p, (int64_t)n); };
    own(&b.shadow2[0], (size_t)b.S);
    own(&b.shadow2[1], (size_t)b.S);
    own(&b.xeval, (size_t)R * D);
    own(&b.h, (size_t)R * H);
    own(&b.z, (size_t)RL * Z);
    own(&b.hd, (size_t)RL * H);
    own(&b.dA, (size_t)RL * b.Dn);
    own(&b.dA1, (size_t)RL * H);
    own(&b.dml, (size_t)R * 2 * Z);
    own(&b.dA3, (size_t)R * H);
    own(&b.ml_slab, (size_t)b.ks_heads * R * 2 * Z);
    own(&b.dz_slab, (size_t)std::max(b.ks_dz, cdiv(H, 256)) * RL * Z);   // (dz fused into dhd: H / 256 slabs)
    own(&b.w_slab, std::max((size_t)b.ks_w1 * Z * H, (size_t)b.ks_w45 * H * 2 * Z));
    own(&b.cp3, (size_t)nrbL * H);
    own(&b.cp45, (size_t)(cdiv(R, bf::kLbRows) + 1) * 2 * Z);
    own(&b.cp1, (size_t)nrbL * H);
    own(&b.cp26, (size_t)nrbL * b.Dn);
    own(&b.lp, (size_t)RL * cdiv(b.Dn, 64));
    own(&b.kl, (size_t)RL * b.nkl);
    own(&b.mu, (size_t)R * Z);
    own(&b.lv, (size_t)R * Z);
    own(&b.eps, (size_t)RL * Z);
    own(&b.elbo_parts, (size_t)2 * bf::kElboBlocks);
    return rc;
}

void bf_free(vaeb_ctx* c) {
    bf::BfState& b = c->bf;
    b.mem.release_all();
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

// ---------------------------------------------------------------- forward
// The 16-byte latent kernels (step_bf16.hpp *_v4): Z % 4 == 0 and every operand they read
// or write with 16-byte accesses 16-byte aligned (else the 4-byte forms; config 5: +6 us).
bool bf_lat4(const bf::LatentArgs& la) {
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
// ... writing the shadow of the weight at shadow offset s
bf::Opt opt_at(bf::Opt o, int64_t s) { o.shadow_out += s; return o; }

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
    const BfMats m = bf_mats(c, par, f.x, M);
    const float* t = c->theta2[par];
    const bool gs = gaussian(c);
    const ArenaSlots& as = c->sl;
    const float *b3 = t + c->off[as.b3], *b4 = t + c->off[as.b4], *b5 = t + c->off[as.b5], *b1 = t + c->off[as.b1],
                *b2 = t + c->off[as.b2], *b6 = gs ? t + c->off[as.b6] : nullptr;
    const float lsc = bf_obj_scale(c);
    // enc: h = tanh(X W3 + b3)
    pr.mark(K_BF_ENC);
    // (256 x 128 tiles with two blocks per CU, as decout: +21 us per step, removed in round 3)
    REP(pr) if (int rc = bf_gemm<bf::KC, bf::KO>(s, m.X, m.W3, M, H, D, 1, bf::EpiBiasAct{b3, 1, M, H, b.h, H}, f.xb)) return rc;
    if (b.thin_h) {
        // heads + latent forward in one launch (thin_bf16.hpp): 64 rows x 64 latents per block
        bf::EpiHeadsLatent eh{};
        eh.b4 = b4; eh.b5 = b5; eh.mu = b.mu; eh.lv = b.lv; eh.eps = b.eps; eh.z = b.z;
        eh.kl_part = b.kl; eh.nkl = b.nkl; eh.M = M; eh.Z = Z; eh.mode = f.mode;
        eh.eps_mode = c->eps_mode == VAEB_EPS_HOST ? 1 : 0; eh.seed = c->seed; eh.step = c->step; eh.domain = f.domain;
        eh.eps_in = f.eps_in; eh.eps_in_ld = f.eps_in_ld;
        eh.rows = f.xb; eh.row_base_mul = f.row_base_mul; eh.row_base_add = f.row_base_add;
        pr.mark(K_BF_HEADS);
        REP(pr) if (int rc = bf_thin<bf::KO, 64>(s, thin_args(m.h, M, m.W45, H, Z), dim3(cdiv(M, 64), Z / 64),
                                                 h16_guarded(c, eh, f.train))) return rc;
    } else {
        // heads: [mu | lv] split-K slabs
        pr.mark(K_BF_HEADS);
        REP(pr) if (int rc = bf_gemm<bf::KC, bf::KO>(s, m.h, m.W45, M, 2 * Z, H, b.ks_heads,
                                                      bf::EpiF32{b.ml_slab, 2 * Z, M, 2 * Z, (int64_t)M * 2 * Z})) return rc;
        // latent: mu, lv, eps, z, KL / LA terms
        bf::LatentArgs la{};
        la.M = M; la.Z = Z; la.L = L; la.est = g.estimator; la.mode = f.mode;
        la.sc = lsc;
        la.ml_slab = b.ml_slab; la.nslab = bf_slices(H, b.ks_heads); la.b4 = b4; la.b5 = b5;
        la.mu = b.mu; la.lv = b.lv; la.eps = b.eps; la.z = b.z; la.kl_part = b.kl;
        la.eps_mode = c->eps_mode == VAEB_EPS_HOST ? 1 : 0; la.seed = c->seed; la.step = c->step; la.domain = f.domain;
        la.eps_in = f.eps_in; la.eps_in_ld = f.eps_in_ld;
        la.rows = f.xb; la.row_base_mul = f.row_base_mul; la.row_base_add = f.row_base_add;
        la = h16_guarded(c, la, f.train);
        pr.mark(K_BF_LATENT);
        if (bf_lat4(la)) REP(pr) hipLaunchKernelGGL(bf::latent_fwd_v4_kernel, dim3(cdiv(M, 8)), dim3(256), 0, s, la);
        else REP(pr) hipLaunchKernelGGL(bf::latent_fwd_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, la);
        CHECK_LAUNCH();
    }
    // dechid: hd = tanh(z W1 + b1) on 256 x 128 tiles, two blocks per CU (K = Z is short: the
    // second block's epilogue overlaps the first's; 743.3 -> 739.8 us per step in round 5)
    pr.mark(K_BF_DECHID);
    REP(pr) if (int rc = bf_gemm_2b<bf::KC, bf::KO>(s, m.z, m.W1, LM, H, Z, bf::EpiBiasAct{b1, 1, LM, H, b.hd, H})) return rc;
    // decout: log p(x|z) partials, dA2 (| dA6), bias partials, y
    pr.mark(K_BF_DECOUT);
    const int nlp = cdiv(Dn, 64);
    // (dA is stored with the backward's loss scale: the fp16 mean objective, h16_scale)
    const float sl = lsc / (float)L * (f.train ? h16_scale(c) : 1.f);
    if (gs) {
        const bf::EpiDecOut<true> e = h16_guarded(
            c, bf::EpiDecOut<true>{b2, b6, f.x, D, M, LM, Dn, D, f.train ? 1 : 0, sl, f.xb, b.dA, Dn, b.lp, nlp, b.cp26, f.yout},
            f.train);
        REP(pr) if (int rc = bf_gemm<bf::KC, bf::KO>(s, m.hd, m.W26, LM, Dn, H, 1, e)) return rc;
    } else {
        // the transposed product a2^T = W2^T hd^T (EpiDecOutT: a lane's four consecutive output
        // columns of one row, 8-byte x / dA accesses through LDS) on the 8-phase 256 x 256
        // tiles, one block per CU (the 256 x 128 two-block form spilled 76 B per lane: 747.6 /
        // 752.2 / 750.4 -> 741.4 / 744.3 / 744.1 us per step, profiles/r5/synth_ab.txt; its
        // switch VAEB_BF_DECT was removed in round 6).  It needs D % 8 == 0 (vaeb_create) and a
        // 16-byte aligned yout (null, or the allocation c->y)
        if (D % 8 != 0 || (reinterpret_cast<uintptr_t>(f.yout) & 15) != 0)
            return fail(VAEB_ERR_ARG, "internal: the Bernoulli decoder launch needs D %% 8 == 0 and a 16-byte aligned output");
        const bf::EpiDecOutT e = h16_guarded(
            c, bf::EpiDecOutT{b2, f.x, D, M, LM, D, f.train ? 1 : 0, sl, f.xb, b.dA, Dn, b.lp, nlp, b.cp26, f.yout, f.xbits},
            f.train);
        const bf::GemmArgs gg = gemm_args(m.W26, m.hd, Dn, LM, H, 256);
        REP(pr) if (int rc = bf_launch8<bf::KO, bf::KC>(s, gg, 1, e)) return rc;
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

// ---------------------------------------------------------------- backward launch groups
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

// A latent-width weight gradient A^T B [M x N] over K rows: split-K slabs into w_slab, then their
// fixed-order sum -> optimizer (opt: the weight's own, opt_at).  Profile slots id_gemm, id_opt.
int bf_wgrad_slabs(vaeb_ctx* c, Prof& pr, hipStream_t s, const Mat& A, const Mat& B, int M, int N, int K, int ks,
                   const bf::ColMap& map, const bf::Opt& opt, KernelId id_gemm, KernelId id_opt) {
    float* slab = c->bf.w_slab;
    pr.mark(id_gemm);
    REP(pr) if (int rc = bf_gemm<bf::KO, bf::KO>(s, A, B, M, N, K, ks, bf::EpiF32{slab, N, M, N, (int64_t)M * N})) return rc;
    bf::WReduceArgs w{};
    w.slab = slab; w.nslab = bf_slices(K, ks); w.M = M; w.N = N;
    w.map = map; w.opt = opt;
    pr.mark(id_opt);
    REP(pr) hipLaunchKernelGGL(bf::wreduce_opt_kernel, dim3(std::min(1024, cdiv((int64_t)M * N, 256))), dim3(256), 0, s, w);
    CHECK_LAUNCH();
    return 0;
}

// [dMu | dLv] from la.ndz dZ slabs (the 16-byte form where bf_lat4 allows it).
int bf_latent_bwd(hipStream_t s, Prof& pr, const bf::LatentArgs& la) {
    if (bf_lat4(la))
        REP(pr) hipLaunchKernelGGL(bf::latent_bwd_v4_kernel, dim3(cdiv(la.M, bf::kLbRows), cdiv(la.Z, 128)), dim3(256), 0, s, la);
    else
        REP(pr) hipLaunchKernelGGL(bf::latent_bwd_kernel, dim3(cdiv(la.M, bf::kLbRows), cdiv(2 * la.Z, 64)), dim3(256), 0, s, la);
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
    const BfStepForm p = bf_step_form(c, prof);
    const bool fork = p.fork, dp = c->comm != nullptr;
    // direct >= 0: the host's minibatch index (vaeb_update), rows addressed from the arguments
    const int64_t row0 = direct >= 0 ? (int64_t)direct * g.B_global + g.row_offset : g.row_offset;
    const bf::BatchRef xb = direct >= 0 ? bf::BatchRef{nullptr, nullptr, 0}
                                        : bf::BatchRef{c->ictl + kCtlOrder, c->ictl, (int64_t)g.B_global * D};
    const bf16_t* x0 = b.x + row0 * D;
    int* const cursor = direct >= 0 ? nullptr : c->ictl;
    const BfMats m = bf_mats(c, par, x0, M);

    BfFwd f{};
    f.Mb = M; f.mode = MODE_TRAIN; f.train = true; f.x = x0; f.xb = xb;
    f.row_base_mul = direct >= 0 ? 0 : g.B_global; f.row_base_add = row0;
    f.eps_in = c->eps_in; f.eps_in_ld = c->eps_rows; f.domain = 0; f.yout = nullptr;
    f.xbits = b.xbits ? b.xbits + row0 * (D / 32) : nullptr;
    if (int rc = bf_forward(c, par, f, pr)) return rc;

    const bf::Opt opt = bf_opt(c, par, !dp, dp || g.keep_grads != 0);
    const ArenaSlots& sl = c->sl;
    // the step's ELBO: result slot, epoch sums, cursor advance
    ElboArgs es = bf_elbo(c, M);
    es.elbo_out = c->elbo_out; es.epoch = c->epoch; es.cursor = cursor; es.step = c->step;
    // DP: replicated Adagrad (+ bf16 shadows) over an all-reduced gradient bucket; sharded DP:
    // dp_fix rewrites the shadow of the theta' shards other ranks updated (gathered before it)
    struct { bf::Opt opt; ElboArgs e; } dx{};
    if (dp) { dx.opt = bf_opt(c, par, true, false); dx.e = es; }
    auto dp_opt = [&](hipStream_t st, const DpRange& r) -> int { return bf_dp_opt_launch(c, st, dx.opt, r, dx.e); };
    auto dp_fix = [&](hipStream_t st, const DpRange& r) -> int { return bf_dp_fix_launch(c, st, dx.opt, r); };
    // dhd: dA1 = ([dA2 | dA6] [W2 | W6]^T) (1 - hd^2)  and  dW2 (| dW6) = hd^T [dA2 | dA6] ->
    // optimizer: both need only the decoder's outputs
    bf::EpiAdagrad e_w26{cmap(gs ? 2 : 0, 0, c->off[sl.W2], gs ? c->off[sl.W6] : 0, D, D), opt_at(opt, b.s26), H, Dn};
    e_w26.vec = adagrad_vec(e_w26);
    const bf::GemmArgs gw2 = gemm_args(m.hd, m.dA, H, Dn, LM, 256);
    if (fork) {
        pr.mark(K_BF_DHD);
        if (p.dhd == DF_T_DZ) {
            // dA1^T = W2 dA^T on 8-phase 256 x 256 tiles, and dZ as split-K slabs from the dA1
            // tile in LDS (EpiDTanhTDz)
            const bf::EpiDTanhTDz e =
                h16_guarded(c, bf::EpiDTanhTDz{{b.hd, H, LM, H, b.dA1, H, b.cp1}, m.W1.p, Z, H, b.dz_slab, (int64_t)LM * Z});
            REP(pr) if (int rc = bf_launch8<bf::KC, bf::KC>(s, gemm_args(m.W26, m.dA, H, LM, Dn, 256), 1, e)) return rc;
        } else if (p.dhd == DF_T) {
            const bf::EpiDTanhT e = h16_guarded(c, bf::EpiDTanhT{b.hd, H, LM, H, b.dA1, H, b.cp1});
            REP(pr) if (int rc = bf_gemm<bf::KC, bf::KC>(s, m.W26, m.dA, H, LM, Dn, 1, e)) return rc;
        } else {
            const bf::EpiDTanh e = h16_guarded(c, bf::EpiDTanh{b.hd, H, LM, H, b.dA1, H, b.cp1});
            REP(pr) if (int rc = bf_gemm<bf::KC, bf::KC>(s, m.dA, m.W26, LM, H, Dn, 1, e)) return rc;
        }
    } else {
        // unforked (profiling, VAEB_BF_FORK=0): dW2 (| dW6) and dhd share one grid of 256 x 256 tiles
        const bf::EpiDTanh e = h16_guarded(c, bf::EpiDTanh{b.hd, H, LM, H, b.dA1, H, b.cp1});
        pr.mark(K_BF_DHD_DW26);
        REP(pr) if (int rc = bf_gemm2<bf::KO, bf::KO, bf::EpiAdagrad, bf::KC, bf::KC, bf::EpiDTanh>(
                        s, gw2, e_w26, gemm_args(m.dA, m.W26, LM, H, Dn, 256), e)) return rc;
    }
    if (dp && !fork) if (int rc = dp_bucket_a(c, pr, dx.opt.th_out, dp_opt, dp_fix)) return rc;
    // dz slabs = dA1 W1^T  (thin: dz + latent backward in one launch, after dW1's fork below)
    if (!p.thin_z && !p.dzf) {
        pr.mark(K_BF_DZ);
        REP(pr) if (int rc = bf_gemm<bf::KC, bf::KC>(s, m.dA1, m.W1, LM, Z, H, b.ks_dz,
                                                      bf::EpiF32{b.dz_slab, Z, LM, Z, (int64_t)LM * Z})) return rc;
    }
    // The second stream forks off right after dhd: dz and dh share the chip with dW2.  (Round 5
    // measured the other fork points and removed them: after dz + [dMu | dLv] +3-5 us per step,
    // after dh +35-40 us, the main chain captured first +13-17 us then.)
    if (fork) {
        HIP_TRY(hipEventRecord(c->fk_ev[0], s));
        HIP_TRY(hipStreamWaitEvent(c->s3, c->fk_ev[0], 0));
        // The second stream's launches (the round-4 order, ELBO_FIRST / W1_FIRST builds removed):
        // the forked dW2 (| dW6) first, so the long product starts earliest, then dW1 (+ its optimizer).
        // (round 5 measured and removed: only the first a of dW2's column tiles forked, the rest in
        // one grid with dW3 after dh -- a = 12 +2-4 us, 8 +10-13, 4 +35 us per step)
        if (int rc = bf_wgrad256(c->s3, gw2, e_w26)) return rc;
        if (dp && c->dp_overlap) {
            // bucket A right behind its gradient, on the fork's stream: reduced (dp_ev[1]) and
            // updated (dp_ev[2]) beside the dz -> dh -> dW3 chain
            if (int rc = dp_reduce_update(c, c->s3, dp_bucket_a_runs(c), dx.opt.th_out, dp_opt, dp_fix, c->dp_ev[1]))
                return rc;
            HIP_TRY(hipEventRecord(c->dp_ev[2], c->s3));
        }
    }
    // dW1 = z^T dA1 (split-K slabs) -> optimizer; unforked: in place on s
    if (int rc = bf_wgrad_slabs(c, pr, p.sw, m.z, m.dA1, Z, H, LM, b.ks_w1, cmap(0, 0, c->off[sl.W1], 0, H, 0),
                                opt_at(opt, b.s1), K_BF_DW1, K_BF_DW1_OPT)) return rc;
    // [dMu | dLv]  (the latent backward's KL / LA terms join the loss-scaled dZ: h16_scale)
    const float bsc = bf_obj_scale(c) * h16_scale(c);
    pr.mark(K_BF_LATENT_BWD);
    if (p.thin_z) {
        bf::EpiDzLatent ez{};
        ez.mu = b.mu; ez.lv = b.lv; ez.eps = b.eps; ez.dmulv = b.dml; ez.colpart = b.cp45;
        ez.sc = bsc; ez.M = M; ez.Z = Z;
        REP(pr) if (int rc = bf_thin<bf::KC, 32>(s, thin_args(m.dA1, M, m.W1, H, -1), dim3(cdiv(M, 32), Z / 128),
                                                 h16_guarded(c, ez))) return rc;
    } else {
        bf::LatentArgs la{};
        la.M = M; la.Z = Z; la.L = L; la.est = g.estimator; la.mode = MODE_TRAIN;
        la.sc = bsc;
        la.mu = b.mu; la.lv = b.lv; la.eps = b.eps;
        // (dz fused: the dhd blocks stored dZ as cdiv(H, 256) split-K slabs)
        la.dz_slab = b.dz_slab; la.ndz = p.dzf ? cdiv(H, 256) : bf_slices(H, b.ks_dz); la.dmulv = b.dml; la.colpart = b.cp45;
        if (int rc = bf_latent_bwd(s, pr, h16_guarded(c, la))) return rc;
    }
    if (fork) {
        HIP_TRY(hipEventRecord(c->fk_ev[2], s));
        HIP_TRY(hipStreamWaitEvent(c->s3, c->fk_ev[2], 0));
    }
    // dh: dA3 = ([dMu | dLv] [W4 | W5]^T) (1 - h^2)
    pr.mark(K_BF_DH);
    if (p.dh == DF_T) {
        // the transposed product dA3^T = [W4 | W5] [dMu | dLv]^T (EpiDTanhT)
        REP(pr) if (int rc = bf_gemm<bf::KC, bf::KC>(s, m.W45, m.dml, H, M, 2 * Z, 1,
                                                      h16_guarded(c, bf::EpiDTanhT{b.h, H, M, H, b.dA3, H, b.cp3}))) return rc;
    } else {
        REP(pr) if (int rc = bf_gemm<bf::KC, bf::KC>(s, m.dml, m.W45, M, H, 2 * Z, 1,
                                                      h16_guarded(c, bf::EpiDTanh{b.h, H, M, H, b.dA3, H, b.cp3}))) return rc;
    }
    // dW4 | dW5 = h^T [dMu | dLv] (split-K slabs) -> optimizer
    if (int rc = bf_wgrad_slabs(c, pr, p.sw, m.h, m.dml, H, 2 * Z, M, b.ks_w45, cmap(1, Z, c->off[sl.W4], c->off[sl.W5], Z, Z),
                                opt_at(opt, b.s45), K_BF_DW45, K_BF_DW45_OPT)) return rc;
    // dW3 = X^T dA3 -> optimizer
    {
        bf::EpiAdagrad e{cmap(0, 0, c->off[sl.W3], 0, H, 0), opt_at(opt, b.s3), D, H};
        e.vec = adagrad_vec(e);
        pr.mark(K_BF_DW3);
        if (fork) {
            // beside the forked dW2 (128 256 x 256 tiles) each product holds half the chip:
            // 256 x 256 tiles here too (ping-pong, the better tile) instead of 256 x 128
            // tiles that the forked dW2's long tiles would leave one round trip of CUs
            if (int rc = bf_wgrad256(s, gemm_args(m.X, m.dA3, D, H, M, 256, 1, xb), e)) return rc;
        } else {
            REP(pr) if (int rc = bf_gemm<bf::KO, bf::KO>(s, m.X, m.dA3, D, H, M, 1, e, xb)) return rc;
        }
    }
    // biases + ELBO
    {
        bf::BiasArgs ba{};
        // (each dtanh epilogue numbers its column-partial rows per the form the plan chose for it)
        const int nrb3 = bf_partial_rows(p.dh, M, H), nrb1 = bf_partial_rows(p.dhd, LM, H);
        ba.seg[0] = bf::BiasSeg{b.cp3, nrb3, H, cmap(0, 0, c->off[sl.b3], 0, 0, 0)};
        ba.seg[1] = bf::BiasSeg{b.cp45, cdiv(M, bf::kLbRows), 2 * Z, cmap(1, Z, c->off[sl.b4], c->off[sl.b5], 0, 0)};
        ba.seg[2] = bf::BiasSeg{b.cp1, nrb1, H, cmap(0, 0, c->off[sl.b1], 0, 0, 0)};
        ba.seg[3] = bf::BiasSeg{b.cp26, bf_partial_rows(DF_AW, LM, Dn), Dn,
                                cmap(gs ? 2 : 0, 0, c->off[sl.b2], gs ? c->off[sl.b6] : 0, 0, 0)};
        ba.nseg = 4;
        ba.total = H + 2 * Z + H + Dn;
        int nbias = 0;
        for (int k = 0; k < 4; ++k) nbias += (ba.segblk[k] = cdiv(ba.seg[k].N, 64));
        ba.opt = opt;
        ElboArgs e = es;
        if (dp) { e.dp_slot = c->grad + c->P; e.elbo_out = nullptr; e.cursor = nullptr; e.step = nullptr; }
        ba.elbo = e;
        ba.elbo_parts = b.elbo_parts; ba.n_elbo_parts = bf::kElboBlocks;
        pr.mark(K_BF_BIAS_ELBO);
        // forked: the ELBO's stage-1 partials on the main stream after dW3: the second stream's tail,
        // not the main chain, ends the step once dz is in dhd (round 5: -2 us against them on
        // the second stream)
        REP(pr) {
            hipLaunchKernelGGL(bf::elbo_partial_kernel, dim3(bf::kElboBlocks), dim3(256), 0, s, e, b.elbo_parts);
            hipLaunchKernelGGL(bf::bias_opt_kernel, dim3(nbias + 1), dim3(256), 0, s, ba);
        }
        CHECK_LAUNCH();
    }
    if (fork) {
        // the forked gradients (dW1, dW45 and, without DP overlap, dW2 | dW6) are bucket B's: join
        // before reducing it (no DP: the step's end)
        HIP_TRY(hipEventRecord(c->fk_ev[1], c->s3));
        HIP_TRY(hipStreamWaitEvent(s, c->fk_ev[1], 0));
    }
    if (dp) if (int rc = dp_bucket_b(c, pr, K_BF_ADAGRAD_DP, dx.opt.th_out, dp_opt, dp_fix)) return rc;
    pr.mark(K_END);
    c->prof_n = pr.k;
    return 0;
}

// ---------------------------------------------------------------- evaluation
// validate / reconstruct for the bf16 engine: one device chunk of bf16 rows x (global
// rows [r0, r0 + rows) for the noise keys and the host eps rows).
int bf_eval_chunk_dev(vaeb_ctx* c, const bf16_t* x, int rows, int64_t r0, int mode, float* out_y) {
    const vaeb_config& g = c->c;
    bf::BfState& b = c->bf;
    const BfFwd f = bf_eval_fwd(c, x, rows, r0, mode, c->eps_in ? c->eps_in + r0 * g.Z : nullptr, 1,
                                (mode == MODE_RECON) ? c->y : nullptr);
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

#include "h16_gemm_hooks.inc"   // vaeb_test_gemm_bf16 / vaeb_bench_gemm_bf16

// vaeb_dp_rank_update (diagnostics): this rank's optimizer launch over `own` and the shadow fix
// over `fr`, the step's own launches (bf_dp_opt_launch / bf_dp_fix_launch) on the context stream
int h16_dp_opt(vaeb_ctx* c, int par, const DpRange& own) { return bf_dp_opt_launch(c, c->s, bf_opt(c, par, true, false), own, ElboArgs{}); }
int h16_dp_fix(vaeb_ctx* c, int par, const DpRange& fr) { return bf_dp_fix_launch(c, c->s, bf_opt(c, par, true, false), fr); }
