// h16_gemm_hooks.inc -- GEMM test / bench hooks of the 16-bit engine (vaeb_test_gemm_bf16 /
// vaeb_bench_gemm_bf16 of include/vaeb_diag.h, on the context's 16-bit type).  Included by
// engine_bf16.inc at its end, so once in each of eng_bf and eng_hf: the launches are the engine's
// own (bf_gemm, bf_launch8, bf_launch on gemm_args).

// f(LA, LB): the operand layouts of the run-time (ako, bko) as compile-time constants.
template <class F>
void with_layouts(int ako, int bko, F&& f) {
    constexpr int kc = bf::KC, ko = bf::KO;
    dispatch<kc, ko>(ako ? ko : kc, [&](auto LA) { dispatch<kc, ko>(bko ? ko : kc, [&](auto LB) { f(LA, LB); }); });
}

// Two K slices combined in the launch (split2_combine): gemm8_body's 64-deep K tiles.
void split2_args(bf::GemmArgs& g, float* part, int* ticket) {
    g.part = part;
    g.ticket = ticket;
    g.kslice = ((cdiv(g.K, 2) + 63) / 64) * 64;
}

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
    DevScratch tmp;   // freed on every return
    int rc = 0;
    rc = rc ? rc : tmp.alloc(&fa, na);
    rc = rc ? rc : tmp.alloc(&fb, nb);
    rc = rc ? rc : tmp.alloc(&ba, na);
    rc = rc ? rc : tmp.alloc(&bb, nb);
    rc = rc ? rc : tmp.alloc(&fc, (int64_t)nz * M * N);
    float* part = nullptr;
    int* ticket = nullptr;
    const int tiles256 = cdiv(M, bf::BM) * cdiv(N, 256);
    if (split2) {
        rc = rc ? rc : tmp.alloc(&part, (int64_t)tiles256 * 65536);
        rc = rc ? rc : tmp.alloc(&ticket, tiles256);
    }
    if (!rc) {
        hipMemcpy(fa, A, na * 4, hipMemcpyHostToDevice);
        hipMemcpy(fb, B, nb * 4, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(bf::to_bf16_kernel, dim3(256), dim3(256), 0, c->s, fa, ba, (int64_t)na);
        hipLaunchKernelGGL(bf::to_bf16_kernel, dim3(256), dim3(256), 0, c->s, fb, bb, (int64_t)nb);
        const bf::EpiF32 e{fc, N, M, N, (int64_t)M * N};
        const Mat a = ako ? mat(ba, K, M) : mat(ba, M, K), b = bko ? mat(bb, K, N) : mat(bb, N, K);
        with_layouts(ako, bko, [&](auto LA, auto LB) {
            constexpr int la = decltype(LA)::value, lb = decltype(LB)::value;
            if (force8) {
                bf::GemmArgs g = gemm_args(a, b, M, N, K, 256, ksplit);
                if (split2) split2_args(g, part, ticket);
                rc = bf_launch8<la, lb>(c->s, g, nz, e);
            } else {
                rc = bf_gemm<la, lb>(c->s, a, b, M, N, K, ksplit, e);
            }
        });
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

// One bench launch on tile width bn (8: 256 x 256 on the 8-phase loop, 9: the same as two K slices).
template <int LA, int LB>
int bench_gemm_launch(hipStream_t s, const bf16_t* A, const bf16_t* B, int M, int N, int K, int bn,
                             const bf::EpiBiasAct& e, float* part, int* ticket) {
    const Mat a = LA == bf::KO ? mat(A, K, M) : mat(A, M, K), b = LB == bf::KO ? mat(B, K, N) : mat(B, N, K);
    bf::GemmArgs g = gemm_args(a, b, M, N, K, bn == 128 ? 128 : 256);
    if (bn == 8 || bn == 9) {
        if (bn == 9) split2_args(g, part, ticket);
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
    DevScratch tmp;   // freed on every return
    int rc = 0;
    if (bn == 9) {
        const int tiles = cdiv(M, bf::BM) * cdiv(N, 256);
        rc = rc ? rc : tmp.alloc(&part, (int64_t)tiles * 65536);
        rc = rc ? rc : tmp.alloc(&ticket, tiles);
    }
    rc = rc ? rc : tmp.alloc(&a, (int64_t)M * K);
    rc = rc ? rc : tmp.alloc(&b, (int64_t)N * K);
    rc = rc ? rc : tmp.alloc(&o, (int64_t)M * N);
    rc = rc ? rc : tmp.alloc(&bias, N);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!rc) {
        hipLaunchKernelGGL(fill_bf16_kernel, dim3(1024), dim3(256), 0, c->s, a, (int64_t)M * K, 1u);
        hipLaunchKernelGGL(fill_bf16_kernel, dim3(1024), dim3(256), 0, c->s, b, (int64_t)N * K, 2u);
        const bf::EpiBiasAct e{bias, 0, M, N, o, N};
        auto one = [&]() {
            int r = 0;
            with_layouts(ako, bko, [&](auto LA, auto LB) {
                r = bench_gemm_launch<decltype(LA)::value, decltype(LB)::value>(c->s, a, b, M, N, K, bn, e, part, ticket);
            });
            return r;
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
    return rc;
}
