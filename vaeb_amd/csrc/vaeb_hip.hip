// vaeb_hip.hip -- C ABI (include/vaeb_hip.h) over the gfx950 SGVB step kernels.
//
// One context = one GPU (one rank).  All state lives in device memory owned here:
// a flat parameter arena in the reference order (VAEB.py:111-115) with matching
// Adagrad-accumulator and gradient arenas, the device-resident training set
// (th.shared x_train, VAEB.py:184), activation/delta buffers, and a small control
// block (batch order, cursor, Philox step, ELBO accumulators) so a step needs no host
// round trip and can be replayed as a hipGraph.
//
// Call map of the host layer (the engines' own maps: engine_f32.inc, engine_bf16.inc, stack_core.inc with
// engine_ae.inc and engine_clf.inc):
//   memory      every device buffer is allocated through a DevOwner (dev_owner.hpp) -- vaeb_ctx::mem,
//               BfState::mem, StackCore::mem -- and freed by its release_all (vaeb_destroy, bf_free,
//               core_close); replaced buffers (data, xval, eps_in, bf.x | xbits | xval) go through
//               drop / replace / grow, a call's scratch through a DevScratch guard.  No hipFree elsewhere.
//   training    vaeb_update -> step_eager;  vaeb_update_many -> [eager first step + order_hook] run_steps
//               (graph replay, or eager) -> enqueue_train_step -> the context's engine.  reset_graphs
//               wherever a captured value or address changes.
//   evaluation  [refusals] -> eval_begin (arena) -> eval_chunks(source, body) -> one read-back:
//     vaeb_validate, vaeb_reconstruct         eval_rows -> eval_pass: eval_chunk_f32 | bf_eval_chunk_dev
//     vaeb_validate_resident                  eval_pass on the resident share -> eval_finish (all-reduce)
//     vaeb_reconstruct_sampled / _full        per chunk and sample sample_chunk_f32 | bf_forward(bf_eval_fwd),
//                                             recon_accum_kernel; copy out and synchronise per chunk
//     vaeb_decode                             decode_chunk_f32 (stages z itself); one synchronise
//     vaeb_encode                             encode_chunk_f32; one synchronise
//     vaeb_marginal_ll(_resident)             iw_pass: iw_chunk_f32 -> eval_acc_read ([all-reduce,] synchronise)
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <type_traits>

#include "../../include/vaeb_diag.h"   // includes vaeb_hip.h
#include "hfuse.hpp"
#include "latent.hpp"
#include "latent_bwd.hpp"
#include "iwae.hpp"
#include "h16_engines.hpp"
#include "ae_mlp.hpp"
#include "ae_iwae.hpp"
#include "ae_corrupt.hpp"
#include "ae_codes.hpp"
#include "clf_softmax.hpp"

using namespace vaeb;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (void)hipGetLastError(); /* a failed call must not resurface at the next launch */ \
            return fail(VAEB_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                               \
        }                                                                                  \
    } while (0)

#define CHECK_LAUNCH()                                                                     \
    do {                                                                                   \
        hipError_t e_ = hipGetLastError();                                                 \
        if (e_ != hipSuccess)                                                              \
            return fail(VAEB_ERR_HIP, "kernel launch failed: %s (%s:%d)",                  \
                        hipGetErrorString(e_), __FILE__, __LINE__);                        \
    } while (0)

inline int r16(int x) { return (x + 15) & ~15; }
inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

template <class T>
int dalloc(T** p, size_t n) {
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e != hipSuccess) return fail(VAEB_ERR_NOMEM, "hipMalloc(%zu) failed: %s", n * sizeof(T), hipGetErrorString(e));
    // the zero fill runs on the null stream, which does not order against the contexts'
    // non-blocking streams: wait for it here, or a kernel enqueued next on a context stream can
    // run before (or beside) the fill and have its stores overwritten with zeros
    e = hipMemset(*p, 0, n * sizeof(T));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(VAEB_ERR_HIP, "zero fill of %zu bytes: %s", n * sizeof(T), hipGetErrorString(e));
    return 0;
}

// Control block layout (ints): [0] cursor, [1] resolved batch, [2..] batch order.
constexpr int kFvParts = 1024;   // FV stream grid (one thetaPrior partial per block)
constexpr int kGraphSteps = 32;  // the longest replayed graph
constexpr int kMaxProfKernels = 24;
constexpr int kDbgWG = 1024;      // diagnostics: stamp slots per launch (workgroups)

// Profile ids (Prof::mark, vaeb_profile_steps) and their names (vaeb_kernel_name), in the same
// order: profiles and bench.py rely on the names, callers of vaeb_profile_steps on the values.
enum KernelId : int {
    K_END = -1,   // closes the last bracket
    K_P1_ENC, K_P2_HEADS, K_P3_DECHID, K_P4_DECOUT, K_P5_DHD_W2, K_P6_DZ,
    K_P7_DH, K_P8_WGRAD_W3W45, K_ALLREDUCE, K_ADAGRAD, K_FV_UPDATE, K_ELBO,
    K_P23_HEADS_DECHID, K_P67_DZ_DH_W1, K_P8_WGRAD_W2, K_P8_WGRAD_W1,
    K_P1_ENC_LATENT, K_P4_DECOUT_Z,
    K_BF_ENC, K_BF_HEADS, K_BF_LATENT, K_BF_DECHID, K_BF_DECOUT, K_BF_DHD, K_BF_DW26,
    K_BF_DZ, K_BF_DW1, K_BF_DW1_OPT, K_BF_LATENT_BWD, K_BF_DH, K_BF_DW45, K_BF_DW45_OPT,
    K_BF_DW3, K_BF_BIAS_ELBO, K_BF_ADAGRAD_DP,
    K_UNUSED35, K_UNUSED36, K_FVS_SAMPLE, K_FVS_UPDATE,
    K_P5_DHD_DZ_W2, K_P8_WGRAD_W3W45W1,
    K_BF_DHD_DW26,
    K_P1_ENC_LATENT_W2, K_P5_DHD_DZ,
    kNumKernelIds
};
const char* kKernelNames[] = {"p1_enc", "p2_heads", "p3_dechid", "p4_decout", "p5_dhd_w2", "p6_dz",
                              "p7_dh", "p8_wgrad_w3w45", "allreduce", "adagrad", "fv_update", "elbo",
                              "p23_heads_dechid", "p67_dz_dh_w1", "p8_wgrad_w2", "p8_wgrad_w1",
                              "p1_enc_latent", "p4_decout_z",
                              // bf16 engine (step_bf16.hpp)
                              "bf_enc", "bf_heads", "bf_latent", "bf_dechid", "bf_decout", "bf_dhd", "bf_dW26",
                              "bf_dz", "bf_dW1", "bf_dW1_opt", "bf_latent_bwd", "bf_dh", "bf_dW45", "bf_dW45_opt",
                              "bf_dW3", "bf_bias_elbo", "bf_adagrad_dp",
                              // weight-sampling full-variational extension (two retired slots first)
                              "unused35", "unused36", "fvs_sample", "fvs_update",
                              // folded latent backward (latent_bwd.hpp)
                              "p5_dhd_dz_w2", "p8_wgrad_w3w45w1",
                              // bf16 engine: dhd and dW2 (| dW6) in one grid
                              "bf_dhd_dW26",
                              // deferred dW2 (round 4): the encoder launch carries the previous
                              // step's dW2 tiles; the dhd launch has none
                              "p1_enc_latent_w2", "p5_dhd_dz"};
static_assert(kNumKernelIds == sizeof(kKernelNames) / sizeof(kKernelNames[0]), "one name per KernelId");
static_assert(K_UNUSED35 == 35 && K_P5_DHD_DZ == 43, "profile ids are part of the ABI");

// Where each parameter sits in c->off (set_arena_layout): the reference order
// W3 W4 W5 W1 W2 [W6] b3 b4 b5 b1 b2 [b6]; W6 / b6 are -1 with the Bernoulli decoder.
struct ArenaSlots {
    int W3, W4, W5, W1, W2, W6, b3, b4, b5, b1, b2, b6;
};

}  // namespace

// DevOwner's one allocation site (dev_owner.hpp): dalloc, registered once the memory exists.
int vaeb::DevOwner::take(void** p, size_t bytes) {
    const int rc = dalloc(reinterpret_cast<char**>(p), bytes);
    if (*p) owned.push_back(*p);
    return rc;
}

struct vaeb_ctx {
    vaeb_config c{};
    hipStream_t s = nullptr;   // every step launch goes to this one stream
    DevOwner mem;              // every device buffer below (interior pointers excepted); vaeb_destroy releases it
    int64_t P = 0;
    int nparams = 0;
    int64_t off[12] = {};   // arena offsets, reference order
    ArenaSlots sl{};        // off's index of each parameter
    // arenas
    float* theta2[2] = {nullptr, nullptr};   // ping-pong parameter arenas
    int par = 0;                              // arena holding the current parameters
    float *acc = nullptr, *grad = nullptr;
    float *fvmu = nullptr, *fvsg = nullptr, *fvam = nullptr, *fvas = nullptr, *fv_part = nullptr;
    float* fvzeta = nullptr;   // VAEB_EST_FVS host-mode weight noise [P]
    // data
    float* data = nullptr;
    int64_t nrows = 0;
    float* xeval = nullptr;
    float* xval = nullptr;        // resident validation set (vaeb_set_valid_data; bf16: bf.xval)
    int64_t nval = 0;
    // control
    int* ictl = nullptr;          // cursor, cur_batch, order[kOrderCap], next (tile_engine.hpp)
    int64_t* step = nullptr;
    float* elbo_out = nullptr;
    double* epoch = nullptr;      // [2] of the control block blk (kernels_aux.hpp kBlk*)
    uint64_t* blk = nullptr;      // epoch [2], status, elbo_out, fixed-point guard word, acc_ml, acc_dz
    double* eval_acc = nullptr;   // [2]
    // noise
    int eps_mode = VAEB_EPS_PHILOX;
    uint64_t seed = 10;
    float* eps_in = nullptr;
    int64_t eps_in_cap = 0, eps_rows = 0;
    // activations
    int cap = 0;                  // padded row capacity (per l plane)
    float *h = nullptr, *mu = nullptr, *lv = nullptr, *eps = nullptr, *z = nullptr, *hd = nullptr,
          *y = nullptr, *dA2 = nullptr, *dA6 = nullptr, *dA1 = nullptr, *dZ = nullptr,
          *dMuLv = nullptr, *dA3 = nullptr, *kl_part = nullptr, *lp_part = nullptr;
    float* yacc = nullptr;        // sampled reconstruction sum (allocated on first use)
    float* iw = nullptr;          // vaeb_marginal_ll scratch (allocated on first use): latent terms
                                  // [cap * L], running (max, sum) [cap][2], row values [cap]
    float *slab_ml = nullptr, *slab_dz = nullptr;  // folded-latent partial slabs (latent.hpp)
    int *cnt_ml = nullptr, *cnt_dz = nullptr;      // their per-row-block arrival counters
    uint64_t *acc_ml = nullptr, *acc_dz = nullptr; // atomic hand-off accumulators (zeroed)
    // host staging (pinned)
    int* h_ctl = nullptr;
    float* h_elbo = nullptr;
    double* h_d2 = nullptr;
    float* h_out = nullptr;       // mapped host [SGVB / B, flags] every training step's last kernel writes
    bool async_pending = false;   // steps enqueued by vaeb_update_many / _async not yet synchronised
    hipEvent_t ctl_ev = nullptr;
    // graphs
    hipGraphExec_t gN[2][kGraphSteps + 1] = {};  // gN[p][n]: n steps from arena p (run_steps)
    bool graph_failed = false;
    std::string graph_err;        // why the capture failed (vaeb_graph_status)
    // comm
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    hipStream_t s3 = nullptr;     // bf16 engine: dW2 (| dW6) + Adagrad forked beside the backward chain
    hipEvent_t fk_ev[3] = {};     // fork after dhd, s3's work done, [dMu | dLv] ready
    int bf_thin = 3;              // VAEB_BF_THIN mask: 1 heads, 2 dz on thin_bf16.hpp (0: split-K + latent kernels)
    bool bf_fork = true;          // VAEB_BF_FORK=0: dW2 in the dhd grid (bf_fuse) or after it
    int bf_dzfuse = 1;            // VAEB_BF_DZFUSE=0: dz + latent backward on the thin launch instead of in the forked dhd
    int bf_dtt = 1;               // VAEB_BF_DTT=0: dhd / dh on A W (EpiDTanh) instead of the transpose (EpiDTanhT)
    hipStream_t s2 = nullptr;     // DP: the gradient buckets' all-reduces and their Adagrad
    hipEvent_t dp_ev[3] = {};     // fork after dW2, bucket A reduced, bucket A updated
    bool dp_overlap = false;      // bucket A on s2 (bf16 engine; VAEB_DP_OVERLAP=0/1 overrides)
    bool dp_shard = false;        // reduce-scatter -> this rank's shard of Adagrad -> all-gather (world > 1)
    bool fold_bwd = true;         // Z <= 32: latent backward folded into the dhd launch (VAEB_FOLD_BWD=0: P67)
    // slab form of the folded backward (fan-in > 16): the dZ slab sum and [dMu | dLv] by
    // reducer workgroups of the LAST launch (kernels_aux.hpp LatRed) instead of a ticket and
    // a last-arriver reducer in the dhd launch.  VAEB_BWD_DEFER=0: the ticketed form.
    bool bwd_defer = true;
    // the deferred dW2: dW2 (| dW6) + Adagrad of step t run in step t+1's encoder launch, on
    // the CUs the encoder leaves idle (latent.hpp enc_latent16_w2_kernel), so the dhd launch
    // holds the dhd tiles alone; host reads of the state flush a pending one first (w2_flush).
    // fp32 LB / LA, no communicator, 16-wave encoder, the latent backward deferred too (ho_dz 2:
    // dw2_deferred).  VAEB_DW2_DEFER=0: dW2 in the dhd launch.
    bool dw2_defer = true;
    bool dw2_paired = false;      // VAEB_DW2_PAIRED=1: always two 32-wide dW2 tiles per workgroup (w2_plan)
    int* w2pend = nullptr;        // device: 1 = a step's dW2 is pending (set by its dhd launch)
    bool w2_dirty = false;        // host: a step was enqueued since the last flush
    bool w2_graph = false;        // host: the captured graphs hold deferred-dW2 steps (run_steps sets w2_dirty)
    int atomic_ho = 1;            // folded latent hand-offs: 1 by fan-in (ho_mode), 0 slabs
    int enc_red = -1;             // encoder slabs summed by the decoder launch: -1 auto, VAEB_ENC_RED=0|1
    // update_many's order upload held back until the eager first step's first launch is out
    // (order_hook): the upload kernel then runs behind the encoder instead of ahead of it
    bool order_pending = false;
    OrderArg order_pend;
    // profiling
    hipEvent_t pev[kMaxProfKernels + 1] = {};
    int prof_n = 0, prof_reps = 1;
    std::vector<int> prof_ids;
    // diagnostics timeline (vaeb_debug_timeline)
    uint64_t* dbg = nullptr;
    int dbg_slot = 0;
    // bf16 large-batch engine (step_bf16.hpp); off for dtype == VAEB_DTYPE_F32
    h16c::BfState bf;
};

namespace {

bool gaussian(const vaeb_ctx* c) { return c->c.decoder == VAEB_DEC_GAUSSIAN; }

// The parameter arena in reference order W3 W4 W5 W1 W2 [W6] b3 b4 b5 b1 b2 [b6]
// (VAEB.py:74-104): c->off, c->sl, c->nparams, c->P from the config alone (no device call).
void set_arena_layout(vaeb_ctx* c) {
    const int64_t D = c->c.D, H = c->c.H, Z = c->c.Z;
    const bool gs = gaussian(c);
    std::vector<int64_t> sz = {D * H, H * Z, H * Z, Z * H, H * D};
    if (gs) sz.push_back(H * D);
    sz.insert(sz.end(), {H, Z, Z, H, D});
    if (gs) sz.push_back(D);
    c->nparams = (int)sz.size();
    int64_t o = 0;
    for (int i = 0; i < c->nparams; ++i) { c->off[i] = o; o += sz[i]; }
    c->P = o;
    int n = 0;   // the slots, in the same order
    ArenaSlots& sl = c->sl;
    sl.W3 = n++; sl.W4 = n++; sl.W5 = n++; sl.W1 = n++; sl.W2 = n++; sl.W6 = gs ? n++ : -1;
    sl.b3 = n++; sl.b4 = n++; sl.b5 = n++; sl.b1 = n++; sl.b2 = n++; sl.b6 = gs ? n++ : -1;
}

// Measurement brackets: mark(id) records an event before launch slot `id`.  With
// reps > 1 (vaeb_profile_steps) every launch of the step is issued `reps` times back to
// back inside its bracket, so bracket time / reps is a kernel's duration plus one
// same-kernel launch gap, free of the event packets' own cost.
#define REP(pr) for (int r_ = 0; r_ < (pr).reps; ++r_)
struct Prof {
    vaeb_ctx* c;
    bool on;
    int reps = 1;
    int k = 0;
    void mark(KernelId id) {
        if (!on) return;
        hipEventRecord(c->pev[k], c->s);
        if (k < (int)c->prof_ids.size()) c->prof_ids[k] = id; else c->prof_ids.push_back(id);
        ++k;
    }
};

// The order upload update_many held back for its eager first step (vaeb_ctx::order_pending):
// launched right after that step's first kernel, or after the step where no launch site
// takes it.  The eager step addresses its rows from its launch arguments and reads neither the
// order nor the cursor, so the upload may run between its launches.
int order_hook(vaeb_ctx* c) {
    if (!c->order_pending) return 0;
    c->order_pending = false;
    hipLaunchKernelGGL(set_order_kernel, dim3(1), dim3(256), 0, c->s, c->ictl, c->order_pend);
    CHECK_LAUNCH();
    return 0;
}

#include "dp_buckets.inc"   // the data-parallel gradient buckets (both engines)
#include "engine_f32.inc"   // the fp32 step engine

// ------------------------------------------------------------------ the 16-bit engine
// One host engine (engine_bf16.inc) over two device instantiations (h16_engines.hpp): bf16
// (VAEB_DTYPE_BF16) and fp16 (VAEB_DTYPE_F16) operands, fp32 accumulation, fp32 masters.
using bf::bf16_t;
bool is_bf16(const vaeb_ctx* c) { return c->c.dtype == VAEB_DTYPE_BF16 || c->c.dtype == VAEB_DTYPE_F16; }   // the 16-bit engine
bool is_f16(const vaeb_ctx* c) { return c->c.dtype == VAEB_DTYPE_F16; }
// A/B (round 3): 256 x 256 tiles on the 8-phase BK = 64 main loop (gemm8_kernel) instead of
// gemm_body's BK = 32 ring, per operand-layout pair: bit (2 LA + LB) of VAEB_BF_GEMM8 (set at
// context creation) -- 1: KC x KC (dhd), 2: KC x KO (enc), 8: KO x KO (dW2, dW3).
int g_gemm8 = 0;
template <int LA, int LB> bool use8() { return (g_gemm8 >> (2 * LA + LB)) & 1; }
// A forward pass of the 16-bit engine for `Mb` rows starting at x (device, 16-bit) with the
// parameters of arena par.  train: store dA / bias partials for the backward.  yout: decoder means.
struct BfFwd {
    int Mb, mode; bool train;
    const bf16_t* x; h16c::BatchRef xb;
    const uint32_t* xbits = nullptr;   // x as bits (binary datasets; the training step's rows), or null
    int64_t row_base_mul, row_base_add;
    const float* eps_in; int64_t eps_in_ld; uint32_t domain;
    float* yout;
};
// An evaluation forward (no stores for a backward) of `rows` rows at x, global rows from r0 (the
// noise keys and the host eps rows), evaluation noise `domain`.
BfFwd bf_eval_fwd(const vaeb_ctx* c, const bf16_t* x, int rows, int64_t r0, int mode, const float* eps_in, uint32_t domain,
                  float* yout) {
    BfFwd f{};
    f.Mb = rows; f.mode = mode; f.train = false; f.x = x; f.xb = h16c::BatchRef{};
    f.row_base_mul = 0; f.row_base_add = r0;
    f.eps_in = eps_in; f.eps_in_ld = c->eps_rows; f.domain = domain;
    f.yout = yout;
    return f;
}
namespace eng_bf {
namespace bf = ::vaeb::bf;
constexpr bool kF16 = false;
#include "engine_bf16.inc"
}  // namespace eng_bf
namespace eng_hf {
namespace bf = ::vaeb::hf;
constexpr bool kF16 = true;
#include "engine_bf16.inc"
}  // namespace eng_hf
#define H16_CALL(fn, ...) (is_f16(c) ? eng_hf::fn(__VA_ARGS__) : eng_bf::fn(__VA_ARGS__))
int bf_train_step(vaeb_ctx* c, int par, bool prof, int direct) { return H16_CALL(bf_train_step, c, par, prof, direct); }
int bf_alloc(vaeb_ctx* c) { return H16_CALL(bf_alloc, c); }
void bf_free(vaeb_ctx* c) { eng_bf::bf_free(c); }   // (type-independent: frees the state's buffers)
int bf_make_shadow(vaeb_ctx* c, int par) { return H16_CALL(bf_make_shadow, c, par); }
int bf_upload_rows(vaeb_ctx* c, const float* x, int64_t n, bf16_t* dst) { return H16_CALL(bf_upload_rows, c, x, n, dst); }
int bf_forward(vaeb_ctx* c, int par, const BfFwd& f, Prof& pr) { return H16_CALL(bf_forward, c, par, f, pr); }
int bf_eval_chunk_dev(vaeb_ctx* c, const bf16_t* x, int rows, int64_t r0, int mode, float* out_y) {
    return H16_CALL(bf_eval_chunk_dev, c, x, rows, r0, mode, out_y);
}
int h16_dp_opt(vaeb_ctx* c, int par, const DpRange& own) { return H16_CALL(h16_dp_opt, c, par, own); }
int h16_dp_fix(vaeb_ctx* c, int par, const DpRange& fr) { return H16_CALL(h16_dp_fix, c, par, fr); }

// One training step of the context's engine (engine_f32.inc enqueue_train_step_f32 for the arguments).
int enqueue_train_step(vaeb_ctx* c, int par, bool prof, bool fresh = true, int direct = -1) {
    return is_bf16(c) ? bf_train_step(c, par, prof, direct) : enqueue_train_step_f32(c, par, prof, fresh, direct);
}

bool flips(const vaeb_ctx* c) { return c->c.estimator != VAEB_EST_FV && c->c.estimator != VAEB_EST_FVS; }

void free_graphs(vaeb_ctx* c) {
    for (auto& fam : c->gN)
        for (auto& gn : fam) {
            if (gn) hipGraphExecDestroy(gn);
            gn = nullptr;
        }
    c->w2_graph = false;
}

// What the captured steps hold by value or by address has changed: drop them, and let the next
// call capture again (a capture that failed before may succeed now).
void reset_graphs(vaeb_ctx* c) {
    free_graphs(c);
    c->graph_failed = false;
}

// Capture nsteps consecutive steps starting from parameter arena `par`.
int capture(vaeb_ctx* c, int nsteps, int par, hipGraphExec_t* out) {
    hipGraph_t gr = nullptr;
    HIP_TRY(hipStreamBeginCapture(c->s, hipStreamCaptureModeThreadLocal));
    int rc = 0;
    // a captured deferred-dW2 step sets w2_dirty as it is recorded; what the host must know is
    // that every REPLAY leaves a dW2 pending: w2_graph, applied by run_steps
    const bool dirty0 = c->w2_dirty;
    c->w2_dirty = false;
    for (int i = 0; i < nsteps && rc == 0; ++i) {
        rc = enqueue_train_step(c, par, false, i == 0);
        if (flips(c)) par ^= 1;
    }
    if (c->w2_dirty) c->w2_graph = true;
    c->w2_dirty = dirty0;
    hipError_t e = hipStreamEndCapture(c->s, &gr);
    if (rc) { if (gr) hipGraphDestroy(gr); return rc; }
    if (e != hipSuccess) return fail(VAEB_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(out, gr, nullptr, nullptr, 0);
    hipGraphDestroy(gr);
    if (e != hipSuccess) return fail(VAEB_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
    // upload now, with the capture: a graph's first launch otherwise pays it inside the call
    // that replays it (the driver's 20-step form replays a graph the warm-up never launched)
    if (hipGraphUpload(*out, c->s) != hipSuccess) (void)hipGetLastError();
    return 0;
}

int step_eager(vaeb_ctx* c, int direct = -1) {
    if (int rc = enqueue_train_step(c, c->par, false, true, direct)) return rc;
    if (flips(c)) c->par ^= 1;
    return 0;
}

// Enqueue n steps (graph replay when enabled, else eager launches).  Graphs: gN[p][m] is m
// steps from arena p (m = 1 .. 32; p = 1 only for the estimators that flip arenas), both
// families captured at the first call (a capture inside a later, timed call would cost more
// than the launches it saves).  A call replays as n / 32 launches of gN[par][32] + ONE launch
// of gN[par][n % 32] from whichever arena it starts: a graph-to-graph boundary leaves the GPU
// idle for ~8 us (kernel trace, profiles/r6/call_timeline.txt), so a 20-step call is one
// graph, not 16 + 4, and the 19 steps after update_many's eager first step are one graph,
// not [one step back to arena 0] + the arena-0 graph (rounds 3-5).
int run_steps(vaeb_ctx* c, int n) {
    if (c->c.use_graph && !c->graph_failed) {
        if (!c->gN[0][1]) {
            int rc = 0;
            for (int p = 0; p < (flips(c) ? 2 : 1); ++p)
                for (int m = 1; m <= kGraphSteps && rc == 0; ++m) rc = capture(c, m, p, &c->gN[p][m]);
            if (rc) {
                // never silent: the reason is kept for vaeb_graph_status.  With a
                // communicator of more than one rank the call fails instead of degrading:
                // single steps (vaeb_update, the first step of a call) are eager at any
                // world size and tested against replay (test_gpu_api.py), but a failed
                // capture there means RCCL could not be captured, and a multi-rank run would
                // then time a launch-bound form nobody asked for
                c->graph_failed = true;
                c->graph_err = g_err;
                free_graphs(c);
                (void)hipGetLastError();
                if (c->comm && c->world > 1)
                    return fail(VAEB_ERR_HIP, "graph capture of the data-parallel step failed at world %d: %s",
                                c->world, c->graph_err.c_str());
            }
        }
        if (!c->graph_failed) {
            // FV / FVS never flip the arena: c->par stays 0 and only family 0 exists
            for (int i = 0; i < n;) {
                const int m = std::min(kGraphSteps, n - i), p = flips(c) ? c->par : 0;
                HIP_TRY(hipGraphLaunch(c->gN[p][m], c->s));
                if (flips(c)) c->par = p ^ (m & 1);
                i += m;
            }
            if (n > 0 && c->w2_graph) c->w2_dirty = true;   // the last replayed step left its dW2 pending
            return 0;
        }
    }
    for (int i = 0; i < n; ++i)
        if (int rc = step_eager(c)) return rc;
    return 0;
}

// Upload a batch order (cursor reset to 0).  Up to kArgOrder entries travel as a kernel
// argument of set_order_kernel (a kernel on the step stream starts sooner than a host ->
// device copy: the fixed cost of a short update_many call), longer ones through the
// pinned staging buffer in one contiguous copy of [cursor, cur_batch, next, order...].
int upload_order(vaeb_ctx* c, const int32_t* idx, int n) {
    if (n <= kArgOrder) {
        OrderArg u;
        u.n = n;
        memcpy(u.v, idx, sizeof(int) * (size_t)n);
        hipLaunchKernelGGL(set_order_kernel, dim3(1), dim3(256), 0, c->s, c->ictl, u);
        CHECK_LAUNCH();
        return 0;
    }
    HIP_TRY(hipEventSynchronize(c->ctl_ev));
    c->h_ctl[0] = 0;
    c->h_ctl[1] = 0;
    c->h_ctl[kCtlNext] = n > 0 ? idx[0] : 0;
    memcpy(c->h_ctl + kCtlOrder, idx, sizeof(int) * (size_t)n);
    HIP_TRY(hipMemcpyAsync(c->ictl, c->h_ctl, sizeof(int) * (size_t)(n + kCtlOrder), hipMemcpyHostToDevice, c->s));
    HIP_TRY(hipEventRecord(c->ctl_ev, c->s));
    return 0;
}

int check_batches(vaeb_ctx* c, const int32_t* idx, int n) {
    if (!c->data) return fail(VAEB_ERR_STATE, "vaeb_set_data has not been called");
    const int64_t nb = c->nrows / c->c.B_global;
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= nb)
            return fail(VAEB_ERR_ARG, "batch index %d out of range [0, %lld)", idx[i], (long long)nb);
    return 0;
}


// ------------------------------------------------------------------ evaluation
// Forward-only passes in chunks of max_eval_rows device rows.  Every call below is
//   [refusals] -> eval_begin (the arena to read) -> eval_chunks(source, body) -> its one read-back,
// and a body hands the chunk to the engine that owns its rows (engine_f32.inc *_chunk_f32,
// engine_bf16.inc bf_eval_chunk_dev / bf_forward): no launch argument is filled here.

// The arena an evaluation reads.  fp32: a pending deferred dW2 flushed first, then the current
// theta, or for VAEB_EST_FVS the posterior mean mu_theta (copied into the spare arena once per
// call).  16-bit: the current arena (no deferred dW2, no FV estimators there).
int eval_begin(vaeb_ctx* c, int* epar) {
    *epar = c->par;
    if (is_bf16(c)) return 0;
    if (int rc = w2_flush(c)) return rc;
    if (c->c.estimator == VAEB_EST_FVS) {
        *epar = c->par ^ 1;
        HIP_TRY(hipMemcpyAsync(c->theta2[*epar], c->fvmu, sizeof(float) * (size_t)c->P, hipMemcpyDeviceToDevice, c->s));
    }
    return 0;
}

// The calls the 16-bit engine does not serve.
int fp32_only(const vaeb_ctx* c, const char* what) {
    return is_bf16(c) ? fail(VAEB_ERR_ARG, "%s is served by fp32 contexts", what) : 0;
}

// This rank's contiguous share of the resident rows: the first (n % world) ranks take one
// extra row (the row split of vaeb_amd/dp.py).
void valid_share(const vaeb_ctx* c, int64_t* lo, int64_t* rows) {
    const int64_t W = c->comm ? c->world : 1, r = c->comm ? c->rank : 0;
    const int64_t base = c->nval / W, extra = c->nval % W;
    *rows = base + (r < extra ? 1 : 0);
    *lo = r * base + std::min<int64_t>(r, extra);
}

// The rows a call walks: host rows x [n x D], staged chunk by chunk through the engine's eval
// buffer; this rank's share of the n = nval resident rows; or (vaeb_decode) n rows that are no
// observations, which the body stages itself.
struct EvalSrc { const float* x; int64_t n; bool resident; };
// One chunk's device rows in the context's engine type (the other pointer is null).
struct EvalRows { const float* f32; const bf16_t* h16; };

// The one chunk loop: body(device rows, rows, r0) for every chunk of at most max_eval_rows rows,
// r0 the chunk's first global row (noise keys, host eps rows, output offsets).  Everything is
// enqueued on the context stream; the synchronises are the caller's.
template <class Body>
int eval_chunks(vaeb_ctx* c, const EvalSrc& src, Body body) {
    const int64_t D = c->c.D, chunk = c->c.max_eval_rows;
    int64_t lo = 0, n = src.n;
    if (src.resident) valid_share(c, &lo, &n);
    for (int64_t r0 = lo; r0 < lo + n; r0 += chunk) {
        const int rows = (int)std::min<int64_t>(chunk, lo + n - r0);
        EvalRows d{};
        if (src.resident) {
            if (is_bf16(c)) d.h16 = c->bf.xval + r0 * D; else d.f32 = c->xval + r0 * D;
        } else if (src.x && is_bf16(c)) {
            if (int rc = bf_upload_rows(c, src.x + r0 * D, rows, c->bf.xeval)) return rc;
            d.h16 = c->bf.xeval;
        } else if (src.x) {
            HIP_TRY(hipMemcpyAsync(c->xeval, src.x + r0 * D, sizeof(float) * (size_t)rows * D, hipMemcpyHostToDevice, c->s));
            d.f32 = c->xeval;
        }
        if (int rc = body(d, rows, r0)) return rc;
    }
    return 0;
}

}  // namespace

// =========================================================================== C ABI
extern "C" {

const char* vaeb_last_error(void) { return g_err.c_str(); }

int vaeb_version(int32_t* major, int32_t* minor) {
    if (major) *major = 0;
    if (minor) *minor = 4;
    return 0;
}

int vaeb_create(const vaeb_config* cfg, vaeb_ctx** out) {
    if (!cfg || !out) return fail(VAEB_ERR_ARG, "null argument");
    const vaeb_config& g = *cfg;
    if (g.D <= 0 || g.H <= 0 || g.Z <= 0 || g.B <= 0 || g.L <= 0)
        return fail(VAEB_ERR_ARG, "dimensions must be positive (D=%d H=%d Z=%d B=%d L=%d)", g.D, g.H, g.Z, g.B, g.L);
    if (g.decoder < 0 || g.decoder > 1 || g.estimator < 0 || g.estimator > 3 || g.objective < 0 || g.objective > 1)
        return fail(VAEB_ERR_ARG, "bad decoder/estimator/objective enum");
    const bool fvx = g.estimator == VAEB_EST_FV || g.estimator == VAEB_EST_FVS;
    if (fvx && g.L != 1)
        return fail(VAEB_ERR_ARG, "the full-variational estimators support L == 1 only (VAEB.py:361)");
    if (g.dtype != VAEB_DTYPE_F32 && g.dtype != VAEB_DTYPE_BF16 && g.dtype != VAEB_DTYPE_F16)
        return fail(VAEB_ERR_ARG, "bad dtype %d", g.dtype);
    if (g.dtype == VAEB_DTYPE_BF16 || g.dtype == VAEB_DTYPE_F16) {
        // (engine_bf16.inc relies on this check: it tests none of D, H, Z % 8 again)
        if (g.D % 8 || g.H % 8 || g.Z % 8)
            return fail(VAEB_ERR_ARG, "bf16 engine: D, H, Z must be multiples of 8 (got %d, %d, %d)", g.D, g.H, g.Z);
        if (g.decoder == VAEB_DEC_GAUSSIAN && g.D % 32)
            return fail(VAEB_ERR_ARG, "bf16 engine: the Gaussian decoder needs D %% 32 == 0 (got %d)", g.D);
        if (fvx) return fail(VAEB_ERR_ARG, "bf16 engine: the FV estimators run on the fp32 path");
        if (g.estimator == VAEB_EST_LA && g.L > 8) return fail(VAEB_ERR_ARG, "bf16 engine: LA supports L <= 8");
    }
    auto* c = new vaeb_ctx();
    c->c = g;
    if (c->c.B_global <= 0) c->c.B_global = g.B;
    if (c->c.adagrad_eps <= 0.f) c->c.adagrad_eps = 1e-6f;
    if (c->c.max_eval_rows <= 0) c->c.max_eval_rows = 10000;
    hipError_t e = hipSetDevice(g.device);
    if (e != hipSuccess) { delete c; return fail(VAEB_ERR_HIP, "hipSetDevice(%d): %s", g.device, hipGetErrorString(e)); }
    e = hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking);
    // Runtime switches (read here only; each alternative is a product path elsewhere or the
    // independent form an agreement test compares the default against -- DESIGN.md 4.4)
    if (const char* fb = getenv("VAEB_FOLD_BWD")) c->fold_bwd = atoi(fb) != 0;
    if (const char* bd = getenv("VAEB_BWD_DEFER")) c->bwd_defer = atoi(bd) != 0;
    if (const char* wd = getenv("VAEB_DW2_DEFER")) c->dw2_defer = atoi(wd) != 0;
    if (const char* wp = getenv("VAEB_DW2_PAIRED")) c->dw2_paired = atoi(wp) != 0;
    if (const char* ah = getenv("VAEB_ATOMIC_HO")) c->atomic_ho = atoi(ah) != 0 ? 1 : 0;
    if (const char* er = getenv("VAEB_ENC_RED")) c->enc_red = atoi(er) != 0 ? 1 : 0;
    if (const char* bk = getenv("VAEB_BF_FORK")) c->bf_fork = atoi(bk) != 0;
    if (const char* tt = getenv("VAEB_BF_DTT")) c->bf_dtt = atoi(tt) != 0;
    if (const char* zf = getenv("VAEB_BF_DZFUSE")) c->bf_dzfuse = atoi(zf) != 0;
    if (const char* bt = getenv("VAEB_BF_THIN")) c->bf_thin = atoi(bt) & 3;
    {
        const char* g8 = getenv("VAEB_BF_GEMM8");
        // default: the 8-phase loop for KC x KC (dhd), KC x KO (enc) and, since round 5, KO x KO
        // (the forked dW2 | dW6 and dW3): round 3 measured KO x KO on it slower (845 vs 816 us);
        // with the round-5 step (dz in dhd, the decoder on the 8-phase loop) it is faster:
        // 738.6 / 741.7 / 740.3 -> 726.8 / 728.7 / 727.4 us (profiles/r5/synth_ab.txt)
        g_gemm8 = g8 ? (int)strtol(g8, nullptr, 0) : 11;
    }
    if (e != hipSuccess) { delete c; return fail(VAEB_ERR_HIP, "stream/event create: %s", hipGetErrorString(e)); }
    const int64_t D = g.D, H = g.H, Z = g.Z;
    set_arena_layout(c);
    c->cap = std::max(r16(g.B), r16(c->c.max_eval_rows));
    const int64_t R = c->cap, RL = (int64_t)c->cap * g.L;
    int rc = 0;
    // every device buffer is registered with c->mem here, where it is allocated (vaeb_destroy releases the list)
    auto own = [&](auto** p, int64_t n) { rc = rc ? rc : c->mem.alloc(p, n); };
    own(&c->theta2[0], c->P);
    own(&c->theta2[1], c->P);
    own(&c->acc, c->P);
    own(&c->grad, c->P + 1);
    if (fvx)
        for (float** p : {&c->fvmu, &c->fvsg, &c->fvam, &c->fvas}) own(p, c->P);
    own(&c->fv_part, kFvParts);
    own(&c->xeval, R * D);
    own(&c->ictl, kCtlOrder + kOrderCap);
    own(&c->step, 1);
    own(&c->eval_acc, 2);
    own(&c->h, R * H);
    own(&c->mu, R * Z);
    own(&c->lv, R * Z);
    own(&c->eps, RL * Z);
    own(&c->z, RL * Z);
    own(&c->hd, RL * H);
    own(&c->y, RL * D);
    // dA6 directly after dA2: the dhd loaders address both through one descriptor (PDhdT)
    own(&c->dA2, RL * D * (gaussian(c) ? 2 : 1));
    if (!rc && gaussian(c)) c->dA6 = c->dA2 + (size_t)RL * D;   // interior pointer: not registered
    own(&c->dA1, RL * H);
    own(&c->dZ, RL * Z);
    own(&c->dMuLv, R * 2 * Z);
    own(&c->dA3, R * H);
    own(&c->kl_part, RL * cdiv(Z, 16));
    own(&c->lp_part, RL * cdiv(D, 16));
    {   // folded-latent slabs and arrival counters (training minibatch only)
        const int64_t Bp = r16(g.B), nctH = cdiv(H, 16);
        own(&c->slab_ml, Bp * nctH * 64);
        own(&c->slab_dz, g.L * Bp * nctH * 32);
        own(&c->cnt_ml, Bp / 16);
        own(&c->cnt_dz, std::max<int64_t>(Bp / 16, kLatCnt * kLatCntStride));
        own(&c->w2pend, 1);
        // one allocation: the guard word the contributors set sits at acc_ml[-1] (latent.hpp fx_inc)
        const int64_t nacc = Bp * 2 * Z * kFxStride;
        own(&c->blk, kBlkAcc + 2 * nacc);
        if (!rc) {   // interior pointers into blk: not registered (the step's result slot blk[kBlkElbo]
                     // is unused: elbo_out is the mapped host slot below)
            c->epoch = reinterpret_cast<double*>(c->blk);
            c->acc_ml = c->blk + kBlkAcc;
            c->acc_dz = c->acc_ml + nacc;
        }
    }
    if (!rc && is_bf16(c)) rc = bf_alloc(c);
    if (!rc && is_bf16(c)) {
        if (hipStreamCreateWithFlags(&c->s3, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->fk_ev[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->fk_ev[1], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->fk_ev[2], hipEventDisableTiming) != hipSuccess)
            rc = fail(VAEB_ERR_HIP, "fork stream / events");
    }
    if (rc) { vaeb_destroy(c); return rc; }
    if (hipHostMalloc((void**)&c->h_ctl, sizeof(int) * (kCtlOrder + kOrderCap), 0) != hipSuccess ||
        hipHostMalloc((void**)&c->h_elbo, sizeof(float) * 4, 0) != hipSuccess ||
        hipHostMalloc((void**)&c->h_d2, sizeof(double) * 4, 0) != hipSuccess) {
        vaeb_destroy(c);
        return fail(VAEB_ERR_NOMEM, "hipHostMalloc failed");
    }
    {
        // the step's scalar result written by the GPU straight into mapped, coherent host
        // memory: vaeb_update reads it with no device -> host copy (and no stream sync)
        void* dp = nullptr;
        if (hipHostMalloc((void**)&c->h_out, sizeof(float) * 4, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer(&dp, c->h_out, 0) != hipSuccess) {
            vaeb_destroy(c);
            return fail(VAEB_ERR_NOMEM, "mapped host ELBO slot");
        }
        memset(c->h_out, 0, sizeof(float) * 4);
        c->elbo_out = static_cast<float*>(dp);
    }
    hipEventCreateWithFlags(&c->ctl_ev, hipEventDisableTiming);
    hipEventRecord(c->ctl_ev, c->s);
    for (auto& ev : c->pev) hipEventCreate(&ev);
    if (hipDeviceSynchronize() != hipSuccess) { vaeb_destroy(c); return fail(VAEB_ERR_HIP, "device init failed"); }
    *out = c;
    return 0;
}

int vaeb_destroy(vaeb_ctx* c) {
    if (!c) return 0;
    if (c->s) hipStreamSynchronize(c->s);
    if (c->s2) hipStreamSynchronize(c->s2);
    if (c->s3) hipStreamSynchronize(c->s3);
    free_graphs(c);
    bf_free(c);
    if (c->comm) ncclCommDestroy(c->comm);
    c->mem.release_all();
    if (c->h_ctl) hipHostFree(c->h_ctl);
    if (c->h_elbo) hipHostFree(c->h_elbo);
    if (c->h_out) hipHostFree(c->h_out);
    if (c->h_d2) hipHostFree(c->h_d2);
    if (c->ctl_ev) hipEventDestroy(c->ctl_ev);
    for (auto& ev : c->pev) if (ev) hipEventDestroy(ev);
    for (auto& ev : c->dp_ev) if (ev) hipEventDestroy(ev);
    for (auto& ev : c->fk_ev) if (ev) hipEventDestroy(ev);
    if (c->s3) hipStreamDestroy(c->s3);
    if (c->s2) hipStreamDestroy(c->s2);
    if (c->s) hipStreamDestroy(c->s);
    delete c;
    return 0;
}

int vaeb_num_params(const vaeb_ctx* c, int64_t* n) {
    if (!c || !n) return fail(VAEB_ERR_ARG, "null argument");
    *n = c->P;
    return 0;
}

int vaeb_set_data(vaeb_ctx* c, const float* x, int64_t n_rows) {
    if (!c || !x || n_rows <= 0) return fail(VAEB_ERR_ARG, "bad data arguments");
    HIP_TRY(hipStreamSynchronize(c->s));
    c->mem.drop(&c->data);
    reset_graphs(c);  // graphs hold the data pointer
    if (is_bf16(c)) {
        // the bf16 engine keeps only a bf16 copy; c->data stays a 16-byte placeholder
        c->bf.mem.drop(&c->bf.x);
        c->bf.mem.drop(&c->bf.xbits);
        // a binary dataset (every value exactly 0 or 1) also as bits, for the Bernoulli decoder
        // epilogue's x tile (EpiDecOutT::load_in): 1/16 of its bytes, the same values
        const int64_t D = c->c.D, nel = n_rows * D;
        bool binary = D % 32 == 0;
        for (int64_t i = 0; binary && i < nel; ++i) binary = x[i] == 0.f || x[i] == 1.f;
        if (binary) {
            std::vector<uint32_t> bits((size_t)(nel / 32), 0u);
            for (int64_t i = 0; i < nel; ++i)
                if (x[i] != 0.f) bits[(size_t)(i >> 5)] |= 1u << (i & 31);
            if (int rc = c->bf.mem.alloc(&c->bf.xbits, (int64_t)bits.size())) return rc;
            HIP_TRY(hipMemcpy(c->bf.xbits, bits.data(), sizeof(uint32_t) * bits.size(), hipMemcpyHostToDevice));
        }
        if (int rc = c->bf.mem.alloc(&c->bf.x, n_rows * c->c.D)) return rc;
        if (int rc = c->mem.alloc(&c->data, 4)) return rc;
        if (int rc = bf_upload_rows(c, x, n_rows, c->bf.x)) return rc;
        HIP_TRY(hipStreamSynchronize(c->s));
        c->nrows = n_rows;
        return 0;
    }
    if (int rc = c->mem.alloc(&c->data, n_rows * c->c.D)) return rc;
    HIP_TRY(hipMemcpy(c->data, x, sizeof(float) * (size_t)n_rows * c->c.D, hipMemcpyHostToDevice));
    c->nrows = n_rows;
    return 0;
}

static int xfer(vaeb_ctx* c, float* dev, const float* hin, float* hout, int64_t n, int64_t want) {
    if (!c || (!hin && !hout)) return fail(VAEB_ERR_ARG, "null argument");
    if (!dev) return fail(VAEB_ERR_STATE, "state not allocated for this estimator");
    if (n != want) return fail(VAEB_ERR_ARG, "size mismatch: got %lld, expected %lld", (long long)n, (long long)want);
    if (int rc = w2_flush(c)) return rc;   // a pending deferred dW2 first: the state is whole
    HIP_TRY(hipStreamSynchronize(c->s));
    if (hin) HIP_TRY(hipMemcpy(dev, hin, sizeof(float) * n, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemcpy(hout, dev, sizeof(float) * n, hipMemcpyDeviceToHost));
    return 0;
}

int vaeb_set_params(vaeb_ctx* c, const float* f, int64_t n) {
    if (int rc = xfer(c, c ? c->theta2[c->par] : nullptr, f, nullptr, n, c ? c->P : 0)) return rc;
    if (is_bf16(c)) {
        if (int rc = bf_make_shadow(c, c->par)) return rc;
        HIP_TRY(hipStreamSynchronize(c->s));
    }
    return 0;
}
int vaeb_get_params(vaeb_ctx* c, float* f, int64_t n) { return xfer(c, c ? c->theta2[c->par] : nullptr, nullptr, f, n, c ? c->P : 0); }
int vaeb_set_adagrad_state(vaeb_ctx* c, const float* f, int64_t n) { return xfer(c, c ? c->acc : nullptr, f, nullptr, n, c ? c->P : 0); }
int vaeb_get_adagrad_state(vaeb_ctx* c, float* f, int64_t n) {
    if (c) if (int rc = dp_gather_acc(c)) return rc;   // sharded DP: a collective (every rank calls)
    return xfer(c, c ? c->acc : nullptr, nullptr, f, n, c ? c->P : 0);
}
int vaeb_get_grads(vaeb_ctx* c, float* f, int64_t n) { return xfer(c, c ? c->grad : nullptr, nullptr, f, n, c ? c->P : 0); }

int vaeb_set_fv_state(vaeb_ctx* c, const float* mu, const float* sg, const float* am, const float* as, int64_t n) {
    int rc = 0;
    rc = rc ? rc : xfer(c, c ? c->fvmu : nullptr, mu, nullptr, n, c ? c->P : 0);
    rc = rc ? rc : xfer(c, c ? c->fvsg : nullptr, sg, nullptr, n, c ? c->P : 0);
    rc = rc ? rc : xfer(c, c ? c->fvam : nullptr, am, nullptr, n, c ? c->P : 0);
    rc = rc ? rc : xfer(c, c ? c->fvas : nullptr, as, nullptr, n, c ? c->P : 0);
    return rc;
}

int vaeb_get_fv_state(vaeb_ctx* c, float* mu, float* sg, float* am, float* as, int64_t n) {
    int rc = 0;
    rc = rc ? rc : xfer(c, c ? c->fvmu : nullptr, nullptr, mu, n, c ? c->P : 0);
    rc = rc ? rc : xfer(c, c ? c->fvsg : nullptr, nullptr, sg, n, c ? c->P : 0);
    rc = rc ? rc : xfer(c, c ? c->fvam : nullptr, nullptr, am, n, c ? c->P : 0);
    rc = rc ? rc : xfer(c, c ? c->fvas : nullptr, nullptr, as, n, c ? c->P : 0);
    return rc;
}

int vaeb_set_eps_mode(vaeb_ctx* c, int32_t mode, uint64_t seed) {
    if (!c || (mode != VAEB_EPS_PHILOX && mode != VAEB_EPS_HOST)) return fail(VAEB_ERR_ARG, "bad eps mode");
    HIP_TRY(hipStreamSynchronize(c->s));
    // captured steps hold the eps mode's kernels and the Philox seed by value (make_args)
    if (mode != c->eps_mode || seed != c->seed) reset_graphs(c);
    c->eps_mode = mode;
    c->seed = seed;
    return 0;
}

int vaeb_push_eps(vaeb_ctx* c, const float* eps, int64_t rows, int32_t L) {
    if (!c || !eps || rows <= 0) return fail(VAEB_ERR_ARG, "bad eps arguments");
    if (L != c->c.L) return fail(VAEB_ERR_ARG, "eps L=%d does not match the model L=%d", L, c->c.L);
    const int64_t n = rows * L * c->c.Z;
    HIP_TRY(hipStreamSynchronize(c->s));
    // (captured steps hold the eps pointer and its row count)
    if (n > c->eps_in_cap || rows != c->eps_rows) reset_graphs(c);
    if (int rc = c->mem.grow(&c->eps_in, &c->eps_in_cap, n)) return rc;
    c->eps_rows = rows;
    HIP_TRY(hipMemcpy(c->eps_in, eps, sizeof(float) * n, hipMemcpyHostToDevice));
    return 0;
}

int vaeb_push_fv_noise(vaeb_ctx* c, const float* zeta, int64_t n) {
    if (!c || !zeta) return fail(VAEB_ERR_ARG, "null argument");
    if (c->c.estimator != VAEB_EST_FVS) return fail(VAEB_ERR_STATE, "weight noise is for the VAEB_EST_FVS estimator");
    if (n != c->P) return fail(VAEB_ERR_ARG, "weight noise needs %lld values (got %lld)", (long long)c->P, (long long)n);
    HIP_TRY(hipStreamSynchronize(c->s));
    if (!c->fvzeta) {
        if (int rc = c->mem.alloc(&c->fvzeta, c->P)) return rc;
        reset_graphs(c);   // captured steps hold the noise pointer
    }
    HIP_TRY(hipMemcpy(c->fvzeta, zeta, sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
    return 0;
}

int vaeb_set_step(vaeb_ctx* c, int64_t step) {
    if (!c) return fail(VAEB_ERR_ARG, "null ctx");
    HIP_TRY(hipStreamSynchronize(c->s));
    HIP_TRY(hipMemcpy(c->step, &step, sizeof(step), hipMemcpyHostToDevice));
    return 0;
}

static int host_eps_ready(vaeb_ctx* c, int64_t rows) {
    if (c->eps_mode == VAEB_EPS_HOST && c->eps_rows != rows)
        return fail(VAEB_ERR_STATE, "host eps mode: pushed %lld rows, step needs %lld (call vaeb_push_eps)",
                    (long long)c->eps_rows, (long long)rows);
    return 0;
}

// Wait until the step's last kernel has written [SGVB / B, flags] into the mapped host slot
// (kernels_aux.hpp elbo_store: flags = 2 | status), polling the slot; the stream is queried
// now and then so that a failed or already-finished stream ends the wait.
static int wait_step_result(vaeb_ctx* c) {
    volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(&c->h_out[1]);
    for (uint64_t spin = 0; *flag == 0u; ++spin) {
        if ((spin & 255) == 255) {
            const hipError_t q = hipStreamQuery(c->s);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return fail(VAEB_ERR_HIP, "step failed: %s", hipGetErrorString(q));
        }
        __builtin_ia32_pause();
    }
    if (*flag == 0u) return fail(VAEB_ERR_STATE, "internal: the step wrote no result");
    return 0;
}

// VAEB_ERR_NUMERIC for the bits of a sticky step status (kernels_aux.hpp kStFxRange, kStF16Range);
// `when`: "the step" / "a step since the last read".
static int numeric_fail(uint64_t st, const char* when) {
    if (st & kStF16Range)
        return fail(VAEB_ERR_NUMERIC, "%s left the fp16 range: a 16-bit operand (z, dA2 | dA6, dA1, [dMu | dLv] or dA3) "
                                      "outside +-65504, NaN or inf; theta and the Adagrad state after it are not "
                                      "usable (restore them, or use VAEB_DTYPE_BF16)", when);
    return fail(VAEB_ERR_NUMERIC, "%s overflowed the fixed-point latent hand-off (a partial outside +-2^17, "
                                  "NaN or inf): its latent values are NaN", when);
}

// The sticky step status read at a sync point (kernels_aux.hpp elbo_emit): cleared, and
// reported as VAEB_ERR_NUMERIC.  st: the step's flag that the status word is set.
static int take_status(vaeb_ctx* c, uint64_t st) {
    if (!st) return 0;
    uint64_t* const h = reinterpret_cast<uint64_t*>(&c->h_d2[3]);
    HIP_TRY(hipMemcpyAsync(h, c->blk + kBlkStatus, sizeof(uint64_t), hipMemcpyDeviceToHost, c->s));
    HIP_TRY(hipMemsetAsync(c->blk + kBlkStatus, 0, sizeof(uint64_t), c->s));
    HIP_TRY(hipStreamSynchronize(c->s));
    return numeric_fail(*h, "the step");
}

int vaeb_update(vaeb_ctx* c, int32_t batch_index, float* out) {
    if (!c) return fail(VAEB_ERR_ARG, "null ctx");
    if (int rc = check_batches(c, &batch_index, 1)) return rc;
    if (int rc = host_eps_ready(c, c->c.B)) return rc;
    // The reference calls update() once per minibatch and waits for its value (VAEB.py:
    // 577-579).  That call is ONE eager step whose minibatch index rides the launch
    // arguments (no order upload, no graph launch), and its value is read from the mapped
    // host slot the step's last kernel writes: 65 -> ~55 us per call (scripts/call_ab.py).
    // Steps still queued from vaeb_update_many / vaeb_update_async would write the mapped
    // slot too: drain them first, so the value read below is this call's step.
    if (c->async_pending) {
        HIP_TRY(hipStreamSynchronize(c->s));
        c->async_pending = false;
    }
    volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(&c->h_out[1]);
    *flag = 0u;
    if (int rc = step_eager(c, batch_index)) return rc;
    if (int rc = wait_step_result(c)) return rc;
    if (out) *out = c->h_out[0];
    return take_status(c, *flag & 1u);
}

int vaeb_update_many(vaeb_ctx* c, const int32_t* idx, int32_t n) {
    if (!c || (!idx && n > 0) || n < 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (int rc = check_batches(c, idx, n)) return rc;
    if (int rc = host_eps_ready(c, c->c.B)) return rc;
    // host eps holds ONE step's noise: a multi-step call would train every step on it
    if (c->eps_mode == VAEB_EPS_HOST && n > 1)
        return fail(VAEB_ERR_STATE, "host eps mode: one step per call (push eps before each vaeb_update)");
    if (n > 0) c->async_pending = true;
    // the call's first step goes out eagerly with its minibatch index in the launch arguments
    // (it reads no order and no cursor): the GPU runs it while the host submits the graph of
    // the remaining steps (which would otherwise lead every call).  The order of those steps
    // is uploaded right behind the step's first launch (order_hook): launched after the whole
    // eager step it started ~6 us after the GPU had finished the step, launched before it the
    // step's first kernel started ~4.5 us after the upload (kernel traces,
    // profiles/r6/call_timeline.txt)
    const bool eager = n >= 2 && c->c.use_graph && c->gN[0][1] && !c->graph_failed && flips(c);
    for (int32_t done = eager ? 1 : 0; done < n;) {
        const int32_t m = std::min<int32_t>(n - done, kOrderCap);
        if (eager && done == 1) {
            if (m <= kArgOrder) {   // the upload rides behind the eager step's first launch
                c->order_pend.n = m;
                memcpy(c->order_pend.v, idx + done, sizeof(int) * (size_t)m);
                c->order_pending = true;
            } else if (int rc = upload_order(c, idx + done, m)) {
                return rc;
            }
            const int rc = step_eager(c, idx[0]);
            const int rh = order_hook(c);   // where the step's launch path took no hook
            if (rc) return rc;
            if (rh) return rh;
        } else if (int rc = upload_order(c, idx + done, m)) {
            return rc;
        }
        if (int rc = run_steps(c, m)) return rc;
        done += m;
    }
    return 0;
}

int vaeb_update_async(vaeb_ctx* c, int32_t batch_index) { return vaeb_update_many(c, &batch_index, 1); }

int vaeb_epoch_elbo(vaeb_ctx* c, double* out_sum, int64_t* out_steps) {
    if (!c) return fail(VAEB_ERR_ARG, "null ctx");
    // epoch sums and the sticky status in one copy, then all three cleared
    HIP_TRY(hipMemcpyAsync(c->h_d2, c->epoch, 3 * sizeof(double), hipMemcpyDeviceToHost, c->s));
    HIP_TRY(hipMemsetAsync(c->epoch, 0, 3 * sizeof(double), c->s));
    HIP_TRY(hipStreamSynchronize(c->s));
    c->async_pending = false;
    if (out_sum) *out_sum = c->h_d2[0];
    if (out_steps) *out_steps = (int64_t)c->h_d2[1];
    uint64_t st;
    memcpy(&st, &c->h_d2[2], sizeof(st));
    return st ? numeric_fail(st, "a step since the last read") : 0;
}

int vaeb_synchronize(vaeb_ctx* c) {
    if (!c) return fail(VAEB_ERR_ARG, "null ctx");
    HIP_TRY(hipStreamSynchronize(c->s));
    c->async_pending = false;
    return 0;
}

// eval_acc[0] on the host, after an optional all-reduce of it over the ranks: the call's
// one stream synchronisation.
static int eval_acc_read(vaeb_ctx* c, bool allreduce, double* out) {
    if (allreduce && c->comm) {
        ncclResult_t r = ncclAllReduce(c->eval_acc, c->eval_acc, 1, ncclDouble, ncclSum, c->comm, c->s);
        if (r != ncclSuccess) return fail(VAEB_ERR_COMM, "ncclAllReduce(validation): %s", ncclGetErrorString(r));
    }
    HIP_TRY(hipMemcpyAsync(c->h_d2, c->eval_acc, 2 * sizeof(double), hipMemcpyDeviceToHost, c->s));
    HIP_TRY(hipStreamSynchronize(c->s));
    *out = c->h_d2[0];
    return 0;
}

// SGVB of n evaluated rows from eval_acc (after an optional all-reduce of it over the
// ranks); the FV estimators add thetaPrior: x.shape[0] * (sum logp + sum KL) + thetaPrior
// (VAEB.py:364).
static int eval_finish(vaeb_ctx* c, int64_t n, bool allreduce, double* out_sum) {
    const vaeb_config& g = c->c;
    double tp = 0.0;
    const bool fvx = g.estimator == VAEB_EST_FV || g.estimator == VAEB_EST_FVS;
    if (fvx) {
        hipLaunchKernelGGL(fv_kernel, dim3(kFvParts), dim3(256), 0, c->s, c->fvmu, c->fvsg, c->fvam, c->fvas, c->P,
                           g.lr, g.adagrad_eps, 0, c->fv_part);
        CHECK_LAUNCH();
        std::vector<float> parts(kFvParts);
        HIP_TRY(hipMemcpyAsync(parts.data(), c->fv_part, sizeof(float) * kFvParts, hipMemcpyDeviceToHost, c->s));
        HIP_TRY(hipStreamSynchronize(c->s));
        for (float p : parts) tp += p;
    }
    double data = 0.0;
    if (int rc = eval_acc_read(c, allreduce, &data)) return rc;
    *out_sum = fvx ? (double)n * data + tp : data;
    return 0;
}

// validate (MODE_EVAL: the chunks' SGVB summed in eval_acc) and reconstruct at z = mu (MODE_RECON:
// the decoder means to out_y, the log-sigma head to out_lv) over src: stream-ordered, one
// synchronise at the end.
static int eval_pass(vaeb_ctx* c, const EvalSrc& src, int mode, float* out_y, double* out_sum, float* out_lv = nullptr) {
    const int64_t D = c->c.D;
    HIP_TRY(hipMemsetAsync(c->eval_acc, 0, 2 * sizeof(double), c->s));
    int epar = 0;
    if (int rc = eval_begin(c, &epar)) return rc;
    if (int rc = eval_chunks(c, src, [&](EvalRows d, int rows, int64_t r0) {
            float* yo = out_y ? out_y + r0 * D : nullptr;
            return d.h16 ? bf_eval_chunk_dev(c, d.h16, rows, r0, mode, yo)
                         : eval_chunk_f32(c, epar, d.f32, rows, r0, mode, yo, out_lv ? out_lv + r0 * D : nullptr);
        }))
        return rc;
    if (mode == MODE_EVAL) return eval_finish(c, src.n, src.resident, out_sum);
    HIP_TRY(hipStreamSynchronize(c->s));
    return 0;
}

static int eval_rows(vaeb_ctx* c, const float* x, int64_t n, int mode, float* out_y, double* out_sum,
                     float* out_lv = nullptr) {
    if (!c || !x || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (mode == MODE_EVAL && c->eps_mode == VAEB_EPS_HOST && c->eps_rows != n)
        return fail(VAEB_ERR_STATE, "host eps mode: validate needs eps for %lld rows (pushed %lld)", (long long)n,
                    (long long)c->eps_rows);
    return eval_pass(c, EvalSrc{x, n, false}, mode, out_y, out_sum, out_lv);
}

int vaeb_validate(vaeb_ctx* c, const float* x, int64_t n, double* out_sum) {
    if (!out_sum) return fail(VAEB_ERR_ARG, "null out_sum");
    return eval_rows(c, x, n, MODE_EVAL, nullptr, out_sum);
}

int vaeb_set_valid_data(vaeb_ctx* c, const float* x, int64_t n) {
    if (!c || !x || n <= 0) return fail(VAEB_ERR_ARG, "bad validation-set arguments");
    HIP_TRY(hipStreamSynchronize(c->s));
    c->nval = 0;
    if (is_bf16(c)) {
        if (int rc = c->bf.mem.replace(&c->bf.xval, n * c->c.D)) return rc;
        if (int rc = bf_upload_rows(c, x, n, c->bf.xval)) return rc;
        HIP_TRY(hipStreamSynchronize(c->s));
    } else {
        if (int rc = c->mem.replace(&c->xval, n * c->c.D)) return rc;
        HIP_TRY(hipMemcpy(c->xval, x, sizeof(float) * (size_t)n * c->c.D, hipMemcpyHostToDevice));
    }
    c->nval = n;
    return 0;
}

int vaeb_validate_resident(vaeb_ctx* c, double* out_sum) {
    if (!c || !out_sum) return fail(VAEB_ERR_ARG, "null argument");
    if (c->nval <= 0) return fail(VAEB_ERR_STATE, "vaeb_set_valid_data has not been called");
    if (c->eps_mode == VAEB_EPS_HOST && c->eps_rows != c->nval)
        return fail(VAEB_ERR_STATE, "host eps mode: resident validation needs eps for all %lld rows (pushed %lld)",
                    (long long)c->nval, (long long)c->eps_rows);
    return eval_pass(c, EvalSrc{nullptr, c->nval, true}, MODE_EVAL, nullptr, out_sum);
}

int vaeb_get_step(vaeb_ctx* c, int64_t* step) {
    if (!c || !step) return fail(VAEB_ERR_ARG, "null argument");
    HIP_TRY(hipStreamSynchronize(c->s));
    HIP_TRY(hipMemcpy(step, c->step, sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

int vaeb_comm_count(vaeb_ctx* c, int32_t* out_world) {
    if (!c || !out_world) return fail(VAEB_ERR_ARG, "null argument");
    if (!c->comm) { *out_world = 1; return 0; }
    int n = 0;
    ncclResult_t r = ncclCommCount(c->comm, &n);
    if (r != ncclSuccess) return fail(VAEB_ERR_COMM, "ncclCommCount: %s", ncclGetErrorString(r));
    *out_world = n;
    return 0;
}

// ------------------------------------------------------------------ native checkpoint
namespace {
struct CkptHeader {
    char magic[8];          // "VAEBCKPT"
    int32_t version;        // 1
    int32_t D, H, Z, L, decoder, estimator, objective, dtype;
    int32_t eps_mode, has_fv;
    int64_t P;
    uint64_t seed;
    int64_t step;
    int64_t reserved[4];
};
constexpr char kCkptMagic[8] = {'V', 'A', 'E', 'B', 'C', 'K', 'P', 'T'};

struct FileCloser { FILE* f; ~FileCloser() { if (f) fclose(f); } };
}  // namespace

int vaeb_checkpoint_save(vaeb_ctx* c, const char* path) {
    if (!c) return fail(VAEB_ERR_ARG, "null argument");
    // path NULL: a non-writing rank of a multi-rank communicator joining the gather;
    // anywhere else it is a caller error, reported before anything runs
    if (!path && !(c->comm && c->world > 1))
        return fail(VAEB_ERR_ARG, "checkpoint: null path (only a non-writing rank of a multi-rank communicator passes NULL)");
    if (int rc = w2_flush(c)) return rc;   // a pending deferred dW2 (vaeb_ctx::dw2_defer)
    if (int rc = dp_gather_acc(c)) return rc;   // sharded DP: the whole Adagrad state (every rank calls)
    if (!path) return 0;
    const vaeb_config& g = c->c;
    CkptHeader h{};
    memcpy(h.magic, kCkptMagic, 8);
    h.version = 1;
    h.D = g.D; h.H = g.H; h.Z = g.Z; h.L = g.L;
    h.decoder = g.decoder; h.estimator = g.estimator; h.objective = g.objective; h.dtype = g.dtype;
    h.eps_mode = c->eps_mode;
    h.has_fv = c->fvmu ? 1 : 0;
    h.P = c->P;
    h.seed = c->seed;
    HIP_TRY(hipStreamSynchronize(c->s));
    HIP_TRY(hipMemcpy(&h.step, c->step, sizeof(int64_t), hipMemcpyDeviceToHost));
    std::vector<float*> arrs = {c->theta2[c->par], c->acc};
    if (h.has_fv) arrs.insert(arrs.end(), {c->fvmu, c->fvsg, c->fvam, c->fvas});
    std::vector<float> buf((size_t)c->P);
    FileCloser fc{fopen(path, "wb")};
    if (!fc.f) return fail(VAEB_ERR_ARG, "checkpoint: cannot open %s for writing", path);
    if (fwrite(&h, sizeof(h), 1, fc.f) != 1) return fail(VAEB_ERR_ARG, "checkpoint: write failed (%s)", path);
    for (float* d : arrs) {
        HIP_TRY(hipMemcpy(buf.data(), d, sizeof(float) * buf.size(), hipMemcpyDeviceToHost));
        if (fwrite(buf.data(), sizeof(float), buf.size(), fc.f) != buf.size())
            return fail(VAEB_ERR_ARG, "checkpoint: write failed (%s)", path);
    }
    if (fflush(fc.f) != 0) return fail(VAEB_ERR_ARG, "checkpoint: flush failed (%s)", path);
    return 0;
}

int vaeb_checkpoint_load(vaeb_ctx* c, const char* path) {
    if (!c || !path) return fail(VAEB_ERR_ARG, "null argument");
    if (int rc = w2_flush(c)) return rc;   // a pending deferred dW2 (vaeb_ctx::dw2_defer)
    const vaeb_config& g = c->c;
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f) return fail(VAEB_ERR_ARG, "checkpoint: cannot open %s", path);
    CkptHeader h{};
    if (fread(&h, sizeof(h), 1, fc.f) != 1 || memcmp(h.magic, kCkptMagic, 8) != 0 || h.version != 1)
        return fail(VAEB_ERR_ARG, "checkpoint: %s is not a version-1 vaeb checkpoint", path);
    if (h.objective != g.objective || h.dtype != g.dtype)
        return fail(VAEB_ERR_ARG, "checkpoint: %s was written by an objective=%d dtype=%d context, this one is "
                    "objective=%d dtype=%d", path, h.objective, h.dtype, g.objective, g.dtype);
    if (h.D != g.D || h.H != g.H || h.Z != g.Z || h.L != g.L || h.decoder != g.decoder ||
        h.estimator != g.estimator || h.P != c->P)
        return fail(VAEB_ERR_ARG, "checkpoint: %s holds a %d-%d-%d L=%d dec=%d est=%d model, the context is "
                    "%d-%d-%d L=%d dec=%d est=%d", path, h.D, h.H, h.Z, h.L, h.decoder, h.estimator,
                    g.D, g.H, g.Z, g.L, g.decoder, g.estimator);
    if (h.has_fv && !c->fvmu) return fail(VAEB_ERR_ARG, "checkpoint: variational state without an FV context");
    std::vector<float> buf((size_t)c->P);
    std::vector<float*> arrs = {c->theta2[c->par], c->acc};
    if (h.has_fv) arrs.insert(arrs.end(), {c->fvmu, c->fvsg, c->fvam, c->fvas});
    HIP_TRY(hipStreamSynchronize(c->s));
    for (float* d : arrs) {
        if (fread(buf.data(), sizeof(float), buf.size(), fc.f) != buf.size())
            return fail(VAEB_ERR_ARG, "checkpoint: %s is truncated", path);
        HIP_TRY(hipMemcpy(d, buf.data(), sizeof(float) * buf.size(), hipMemcpyHostToDevice));
    }
    if (is_bf16(c)) {
        if (int rc = bf_make_shadow(c, c->par)) return rc;
        HIP_TRY(hipStreamSynchronize(c->s));
    }
    HIP_TRY(hipMemcpy(c->step, &h.step, sizeof(int64_t), hipMemcpyHostToDevice));
    // captured steps hold the eps mode's kernels and the Philox seed by value (make_args)
    if (h.eps_mode != c->eps_mode || h.seed != c->seed) reset_graphs(c);
    c->eps_mode = h.eps_mode;
    c->seed = h.seed;
    return 0;
}

int vaeb_reconstruct(vaeb_ctx* c, const float* x, int64_t n, float* out_y) {
    return vaeb_reconstruct_full(c, x, n, 0, out_y, nullptr);
}

int vaeb_reconstruct_sampled(vaeb_ctx* c, const float* x, int64_t n, int32_t n_samples, float* out_y) {
    return vaeb_reconstruct_full(c, x, n, n_samples, out_y, nullptr);
}

// VAEB.reconstruct (VAEB.py:267-291) before its closing multivariate_normal draw: the
// decoder outputs at z = mu (n_samples <= 0) or averaged over n_samples posterior draws
// z_s = mu + exp(lv / 2) eps_s, summed on device in sample order (:279-291).  eps_s:
// Philox stream s + 1 of the validation domain, or (host eps mode) rows [s * n, (s + 1) * n)
// of the pushed eps.  out_lv (Gaussian decoder, fp32 engine): the log-sigma head, averaged
// the same way (:284, 289) -- the caller's draw is y_mu + exp(y_log_sigma) * N(0, 1) (:295-297).
int vaeb_reconstruct_full(vaeb_ctx* c, const float* x, int64_t n, int32_t n_samples, float* out_y, float* out_lv) {
    if (!c || !x || n <= 0 || !out_y) return fail(VAEB_ERR_ARG, "bad arguments");
    if (out_lv && !gaussian(c)) return fail(VAEB_ERR_ARG, "the log-sigma head exists for the Gaussian decoder only");
    if (out_lv) if (int rc = fp32_only(c, "the log-sigma output")) return rc;
    if (n_samples <= 0) return eval_rows(c, x, n, MODE_RECON, out_y, nullptr, out_lv);
    const bool host = c->eps_mode == VAEB_EPS_HOST;
    if (host && c->eps_rows != n * n_samples)
        return fail(VAEB_ERR_STATE, "host eps mode: sampled reconstruct needs eps for %lld rows (n * n_samples), pushed %lld",
                    (long long)(n * n_samples), (long long)c->eps_rows);
    const vaeb_config& g = c->c;
    const int64_t nacc = (int64_t)g.max_eval_rows * g.D;
    if (int rc = c->mem.lazy(&c->yacc, nacc * (gaussian(c) ? 2 : 1))) return rc;
    float* lacc = gaussian(c) ? c->yacc + nacc : nullptr;   // (interior pointer)
    int epar = 0;
    if (int rc = eval_begin(c, &epar)) return rc;
    // per chunk: the samples' decoder outputs summed in yacc (| lacc), copied out, one synchronise
    return eval_chunks(c, EvalSrc{x, n, false}, [&](EvalRows d, int rows, int64_t r0) {
        const int64_t ny = (int64_t)rows * g.D;
        for (int sidx = 0; sidx < n_samples; ++sidx) {
            const uint32_t domain = 1u | ((uint32_t)(sidx + 1) << 1);
            const float* eps = (host && c->eps_in) ? c->eps_in + ((int64_t)sidx * n + r0) * g.Z : nullptr;
            Prof pr{c, false};
            if (int rc = d.h16 ? bf_forward(c, epar, bf_eval_fwd(c, d.h16, rows, r0, MODE_EVAL, eps, domain, c->y), pr)
                               : sample_chunk_f32(c, epar, d.f32, rows, r0, domain, eps))
                return rc;
            const float scale = (sidx == n_samples - 1) ? (float)n_samples : 0.f;
            const dim3 grid((unsigned)std::min<int64_t>(1024, cdiv(ny, 256)));
            hipLaunchKernelGGL(recon_accum_kernel, grid, dim3(256), 0, c->s, c->yacc, c->y, ny, sidx == 0 ? 1 : 0, scale);
            CHECK_LAUNCH();
            if (out_lv) {
                hipLaunchKernelGGL(recon_accum_kernel, grid, dim3(256), 0, c->s, lacc, c->dA6, ny, sidx == 0 ? 1 : 0, scale);
                CHECK_LAUNCH();
            }
        }
        HIP_TRY(hipMemcpyAsync(out_y + r0 * g.D, c->yacc, sizeof(float) * (size_t)ny, hipMemcpyDeviceToHost, c->s));
        if (out_lv)
            HIP_TRY(hipMemcpyAsync(out_lv + r0 * g.D, lacc, sizeof(float) * (size_t)ny, hipMemcpyDeviceToHost, c->s));
        HIP_TRY(hipStreamSynchronize(c->s));
        return 0;
    });
}

// The decoder from a given z (freyFace.py:173-187 `image(z)`, compiled at :237-245; VAEB.py
// :253-265): hd = tanh(z W1 + b1), mu = sigmoid(hd W2 + b2), and for the Gaussian decoder the
// log-sigma head hd W6 + b6 (out_lv).  fp32 contexts; z is [n x Z] row-major.
int vaeb_decode(vaeb_ctx* c, const float* z, int64_t n, float* out_mu, float* out_lv) {
    if (!c || !z || n <= 0 || !out_mu) return fail(VAEB_ERR_ARG, "bad arguments");
    if (out_lv && !gaussian(c)) return fail(VAEB_ERR_ARG, "the log-sigma head exists for the Gaussian decoder only");
    if (int rc = fp32_only(c, "vaeb_decode")) return rc;
    const vaeb_config& g = c->c;
    int epar = 0;
    if (int rc = eval_begin(c, &epar)) return rc;
    if (int rc = eval_chunks(c, EvalSrc{nullptr, n, false}, [&](EvalRows, int rows, int64_t r0) {
            return decode_chunk_f32(c, epar, z + r0 * g.Z, rows, out_mu + r0 * g.D, out_lv ? out_lv + r0 * g.D : nullptr);
        }))
        return rc;
    HIP_TRY(hipStreamSynchronize(c->s));
    return 0;
}

// ------------------------------------------------------------------ encoder outputs, IWAE bound
int vaeb_encode(vaeb_ctx* c, const float* x, int64_t n, float* out_mu, float* out_lv) {
    if (!c || !x || n <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (int rc = fp32_only(c, "vaeb_encode")) return rc;
    const vaeb_config& g = c->c;
    int epar = 0;
    if (int rc = eval_begin(c, &epar)) return rc;
    if (int rc = eval_chunks(c, EvalSrc{x, n, false}, [&](EvalRows d, int rows, int64_t r0) {
            if (int rc = encode_chunk_f32(c, epar, d.f32, rows, r0, nullptr)) return rc;
            const size_t nb = sizeof(float) * (size_t)rows * g.Z;
            if (out_mu) HIP_TRY(hipMemcpyAsync(out_mu + r0 * g.Z, c->mu, nb, hipMemcpyDeviceToHost, c->s));
            if (out_lv) HIP_TRY(hipMemcpyAsync(out_lv + r0 * g.Z, c->lv, nb, hipMemcpyDeviceToHost, c->s));
            return 0;
        }))
        return rc;
    HIP_TRY(hipStreamSynchronize(c->s));
    return 0;
}

// The K-sample importance-weighted sum over src (fp32 contexts): argument / state checks, the
// lazily allocated scratch, the chunks, and eval_acc read once at the end (resident rows:
// all-reduced over the ranks).  The pushed eps must cover src.n rows K times.
static int iw_pass(vaeb_ctx* c, const EvalSrc& src, int32_t K, double* out_sum, float* out_rows) {
    if (K < 1 || K > (1 << 20))
        return fail(VAEB_ERR_ARG, "K = %d: 1 to 2^20 samples (the Philox sample-stream field)", K);
    if (c->eps_mode == VAEB_EPS_HOST && c->eps_rows != src.n * K)
        return fail(VAEB_ERR_STATE, "host eps mode: the marginal likelihood needs eps for %lld rows (n * K), pushed %lld",
                    (long long)(src.n * K), (long long)c->eps_rows);
    if (int rc = c->mem.lazy(&c->iw, (int64_t)c->cap * (c->c.L + 3))) return rc;
    HIP_TRY(hipMemsetAsync(c->eval_acc, 0, 2 * sizeof(double), c->s));
    int epar = 0;
    if (int rc = eval_begin(c, &epar)) return rc;
    if (int rc = eval_chunks(c, src, [&](EvalRows d, int rows, int64_t r0) {
            return iw_chunk_f32(c, epar, d.f32, rows, r0, K, c->eps_in ? c->eps_in + r0 * c->c.Z : nullptr, src.n,
                                out_rows ? out_rows + r0 : nullptr);
        }))
        return rc;
    return eval_acc_read(c, src.resident, out_sum);
}

int vaeb_marginal_ll(vaeb_ctx* c, const float* x, int64_t n, int32_t K, double* out_sum, float* out_rows) {
    if (!c || !x || n <= 0 || !out_sum) return fail(VAEB_ERR_ARG, "bad arguments");
    if (int rc = fp32_only(c, "vaeb_marginal_ll")) return rc;
    return iw_pass(c, EvalSrc{x, n, false}, K, out_sum, out_rows);
}

int vaeb_marginal_ll_resident(vaeb_ctx* c, int32_t K, double* out_sum) {
    if (!c || !out_sum) return fail(VAEB_ERR_ARG, "null argument");
    if (int rc = fp32_only(c, "vaeb_marginal_ll_resident")) return rc;
    if (c->nval <= 0) return fail(VAEB_ERR_STATE, "vaeb_set_valid_data has not been called");
    return iw_pass(c, EvalSrc{nullptr, c->nval, true}, K, out_sum, nullptr);
}

int vaeb_comm_unique_id(uint8_t out_id[128]) {
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(VAEB_ERR_COMM, "ncclGetUniqueId: %s", ncclGetErrorString(r));
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(out_id, &id, 128);
    return 0;
}

int vaeb_comm_init(vaeb_ctx* c, const uint8_t id_bytes[128], int32_t rank, int32_t world) {
    if (!c || !id_bytes || world <= 0 || rank < 0 || rank >= world) return fail(VAEB_ERR_ARG, "bad comm arguments");
    if (int rc = w2_flush(c)) return rc;   // a pending deferred dW2 (vaeb_ctx::dw2_defer)
    if ((c->c.estimator == VAEB_EST_FV && world > 1) || c->c.estimator == VAEB_EST_FVS)
        return fail(VAEB_ERR_ARG, "the full-variational paths are single-rank");
    if (c->comm) return fail(VAEB_ERR_STATE, "communicator already initialised");
    HIP_TRY(hipSetDevice(c->c.device));
    // Bucket A's all-reduce + Adagrad on a second stream beside the backward, where the
    // window it can hide behind is longer than what the fork costs.  The graph's fork and
    // join cost ~19 us per step whatever the world size (fp32 MNIST at world 1: 66.0 vs
    // 47.1 us, profiles/r3/dp_world1_start.txt), and on the fp32 engine the backward left
    // after dW2 (| dW6) is the one last launch, ~10 us: at most 10 us of all-reduce could
    // hide there at ANY world size, so the fp32 step never forks.  On the bf16 engine
    // (config 5) the window is ~500 us and bucket A (34 MB) alone is worth the fork at
    // world 1 already (933 vs ~940 us per step), so it always forks.
    c->dp_overlap = is_bf16(c);
    if (const char* ov = getenv("VAEB_DP_OVERLAP")) c->dp_overlap = atoi(ov) != 0;
    // sharded optimizer at world > 1 (dp_reduce_update); VAEB_DP_SHARD=1 forces it at world 1 (tests)
    c->dp_shard = world > 1;
    if (const char* sh = getenv("VAEB_DP_SHARD")) c->dp_shard = atoi(sh) != 0;
    if (!c->s2) {
        HIP_TRY(hipStreamCreateWithFlags(&c->s2, hipStreamNonBlocking));
        for (auto& ev : c->dp_ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    ncclUniqueId id;
    memcpy(&id, id_bytes, 128);
    ncclResult_t r = ncclCommInitRank(&c->comm, world, id, rank);
    if (r != ncclSuccess) return fail(VAEB_ERR_COMM, "ncclCommInitRank: %s", ncclGetErrorString(r));
    c->rank = rank;
    c->world = world;
    reset_graphs(c);
    return 0;
}

static const struct { const char* name; int which; } kActs[] = {
    {"h", 0}, {"mu", 1}, {"lv", 2}, {"eps", 3}, {"z", 4}, {"hd", 5}, {"dA2", 6}, {"dA6", 7},
    {"dA1", 8}, {"dZ", 9}, {"dMuLv", 10}, {"dA3", 11}, {"y", 12}, {"kl_part", 13}, {"lp_part", 14}};

int vaeb_get_activation(vaeb_ctx* c, const char* name, float* out, int64_t n) {
    if (!c || !name || !out) return fail(VAEB_ERR_ARG, "null argument");
    float* ptrs[] = {c->h, c->mu, c->lv, c->eps, c->z, c->hd, c->dA2, c->dA6, c->dA1, c->dZ, c->dMuLv, c->dA3, c->y,
                     c->kl_part, c->lp_part};
    if (strcmp(name, "dZ") == 0 && fused_latent(c) && c->fold_bwd && !is_bf16(c) && ho_dz(c) == 1)
        return fail(VAEB_ERR_STATE, "dZ is not stored by the atomic latent hand-off (fan-in <= 16, latent_bwd.hpp): "
                                    "create the context with VAEB_ATOMIC_HO=0 to read it");
    const int64_t R = c->cap, RL = (int64_t)c->cap * c->c.L, D = c->c.D, H = c->c.H, Z = c->c.Z;
    const int64_t cap[] = {R * H, R * Z, R * Z, RL * Z, RL * Z, RL * H, RL * D, RL * D, RL * H, RL * Z, R * 2 * Z,
                           R * H, RL * D, RL * cdiv(Z, 16), RL * cdiv(D, 16)};
    for (auto& a : kActs)
        if (strcmp(a.name, name) == 0) {
            if (!ptrs[a.which]) return fail(VAEB_ERR_STATE, "activation %s not allocated", name);
            if (n < 0 || n > cap[a.which])
                return fail(VAEB_ERR_ARG, "activation %s holds %lld floats, %lld requested", name,
                            (long long)cap[a.which], (long long)n);
            HIP_TRY(hipStreamSynchronize(c->s));
            HIP_TRY(hipMemcpy(out, ptrs[a.which], sizeof(float) * n, hipMemcpyDeviceToHost));
            return 0;
        }
    return fail(VAEB_ERR_ARG, "unknown activation '%s'", name);
}

int vaeb_profile_steps(vaeb_ctx* c, int32_t n_steps, float* out_ms, int32_t* out_ids, int32_t max_k,
                       int32_t* out_nk) {
    if (!c || !out_ms || n_steps <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    if (int rc = w2_flush(c)) return rc;
    if (!c->data) return fail(VAEB_ERR_STATE, "no data");
    constexpr int kReps = 8;   // each launch issued 8x back to back inside its event bracket
    std::vector<int32_t> order((size_t)n_steps * kReps);
    const int64_t nb = c->nrows / c->c.B_global;
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)(i % nb);
    if (int rc = upload_order(c, order.data(), (int)order.size())) return rc;
    std::vector<double> tot(kMaxProfKernels, 0.0);
    c->prof_reps = kReps;
    for (int it = 0; it < n_steps; ++it) {
        // 1 ms hold: the eager launches queue up behind it (no host-launch gaps)
        hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(64), 0, c->s, (uint64_t)100000);
        CHECK_LAUNCH();
        int rc = enqueue_train_step(c, c->par, true);
        if (rc) { c->prof_reps = 1; return rc; }
        if (flips(c)) c->par ^= 1;   // repeats all read arena par and write par ^ 1
        HIP_TRY(hipStreamSynchronize(c->s));
        for (int k = 0; k + 1 < c->prof_n; ++k) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, c->pev[k], c->pev[k + 1]));
            tot[k] += ms / kReps;
        }
    }
    c->prof_reps = 1;
    const int nk = std::max(0, c->prof_n - 1);
    for (int k = 0; k < nk && k < max_k; ++k) {
        out_ms[k] = (float)(tot[k] / n_steps);
        if (out_ids) out_ids[k] = c->prof_ids[k];
    }
    if (out_nk) *out_nk = nk;
    return 0;
}

int vaeb_debug_timeline(vaeb_ctx* c, int32_t batch_index, uint64_t* out, int64_t cap, int32_t* out_launches) {
    if (!c || !out) return fail(VAEB_ERR_ARG, "bad arguments");
    if (int rc = w2_flush(c)) return rc;
    if (int rc = check_batches(c, &batch_index, 1)) return rc;
    const size_t n = (size_t)kMaxProfKernels * kDbgWG * 8;
    DevScratch tmp;   // the stamp buffer: this call's own, freed on every return
    uint64_t* d = nullptr;
    if (int rc = tmp.alloc(&d, (int64_t)n)) return rc;
    HIP_TRY(hipMemsetAsync(d, 0, n * sizeof(uint64_t), c->s));
    if (int rc = upload_order(c, &batch_index, 1)) return rc;
    c->dbg = d;        // the context points at it for this one step only:
    c->dbg_slot = 0;   // later steps (and captured graphs) run without stamps
    const int rc = enqueue_train_step(c, c->par, false);
    if (flips(c)) c->par ^= 1;
    const int launches = c->dbg_slot;
    c->dbg_slot = 0;
    c->dbg = nullptr;
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->s));
    const size_t m = std::min<size_t>(n, (size_t)cap);
    HIP_TRY(hipMemcpy(out, d, m * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (out_launches) *out_launches = launches;
    return 0;
}

int vaeb_test_gemm_bf16(vaeb_ctx* c, int32_t ako, int32_t bko, int32_t M, int32_t N, int32_t K, const float* A,
                        const float* B, float* C, int32_t ksplit) {
    if (!c) return fail(VAEB_ERR_ARG, "null ctx");
    return is_f16(c) ? eng_hf::h16_test_gemm(c, ako, bko, M, N, K, A, B, C, ksplit)
                     : eng_bf::h16_test_gemm(c, ako, bko, M, N, K, A, B, C, ksplit);
}

int vaeb_bench_gemm_bf16(vaeb_ctx* c, int32_t ako, int32_t bko, int32_t M, int32_t N, int32_t K, int32_t bn,
                         int32_t reps, float* out_ms) {
    if (!c) return fail(VAEB_ERR_ARG, "null ctx");
    return is_f16(c) ? eng_hf::h16_bench_gemm(c, ako, bko, M, N, K, bn, reps, out_ms)
                     : eng_bf::h16_bench_gemm(c, ako, bko, M, N, K, bn, reps, out_ms);
}

int vaeb_time_update_many(vaeb_ctx* c, const int32_t* idx, int32_t n, float* out_gpu_ms, double* out_enqueue_ms) {
    if (!c || !out_gpu_ms) return fail(VAEB_ERR_ARG, "null argument");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipStreamSynchronize(c->s));
    HIP_TRY(hipEventRecord(e0, c->s));
    const auto t0 = std::chrono::steady_clock::now();
    int rc = vaeb_update_many(c, idx, n);
    const auto t1 = std::chrono::steady_clock::now();
    if (rc == 0) {
        hipEventRecord(e1, c->s);
        hipEventSynchronize(e1);
        hipEventElapsedTime(out_gpu_ms, e0, e1);
        if (out_enqueue_ms) *out_enqueue_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return rc;
}

int vaeb_busy(vaeb_ctx* c, int32_t us) {
    if (!c || us <= 0) return fail(VAEB_ERR_ARG, "bad arguments");
    hipLaunchKernelGGL(busy_kernel, dim3(2048), dim3(256), 0, c->s, (uint64_t)us * 100, c->fv_part);
    CHECK_LAUNCH();
    return 0;
}

int vaeb_graph_status(vaeb_ctx* c, int32_t* mode, char* msg, int32_t cap) {
    if (!c || !mode) return fail(VAEB_ERR_ARG, "null argument");
    if (!c->c.use_graph) *mode = VAEB_GRAPH_OFF;
    else if (c->graph_failed) *mode = VAEB_GRAPH_EAGER_FALLBACK;
    else *mode = c->gN[0][1] ? VAEB_GRAPH_REPLAY : VAEB_GRAPH_NOT_CAPTURED;
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", c->graph_failed ? c->graph_err.c_str() : "");
    return 0;
}

int vaeb_comm_info(vaeb_ctx* c, int32_t* rccl_version, int32_t* dp_overlap, int32_t* world) {
    if (!c) return fail(VAEB_ERR_ARG, "null ctx");
    if (rccl_version) {
        int v = 0;
        ncclResult_t r = ncclGetVersion(&v);
        if (r != ncclSuccess) return fail(VAEB_ERR_COMM, "ncclGetVersion: %s", ncclGetErrorString(r));
        *rccl_version = v;
    }
    if (dp_overlap) *dp_overlap = c->comm ? (c->dp_overlap ? 1 : 0) : -1;
    if (world) *world = c->comm ? c->world : 1;
    return 0;
}

int vaeb_dp_plan(const vaeb_config* cfg, int32_t world, int32_t rank, int32_t sharded, int32_t bucket,
                 int64_t* out_P, int64_t* runs, int32_t* out_nrun, int64_t* own, int32_t* out_nown, int32_t* out_book,
                 int64_t* foreign, int32_t* out_nforeign) {
    if (!cfg || world <= 0 || rank < 0 || rank >= world || bucket < 0 || bucket > 2)
        return fail(VAEB_ERR_ARG, "bad plan arguments");
    if (cfg->D <= 0 || cfg->H <= 0 || cfg->Z <= 0) return fail(VAEB_ERR_ARG, "dimensions must be positive");
    // a host-only context holding exactly the fields the plan functions read (no stream, no
    // allocation): the same code dp_reduce_update runs on a rank
    vaeb_ctx c;
    c.c = *cfg;
    set_arena_layout(&c);
    c.world = world;
    c.rank = rank;
    c.dp_shard = sharded != 0;
    const DpBucket bk = bucket == 0 ? dp_bucket_a_runs(&c) : bucket == 1 ? dp_bucket_b_runs(&c) : dp_bucket_all_runs(&c);
    if (out_P) *out_P = c.P;
    if (runs)
        for (int j = 0; j < bk.nrun; ++j) {
            runs[3 * j] = bk.lo[j];
            runs[3 * j + 1] = bk.n[j];
            runs[3 * j + 2] = dp_shard_len(&c, bk.n[j]);
        }
    if (out_nrun) *out_nrun = bk.nrun;
    auto put = [](const DpRange& r, int64_t* dst, int32_t* cnt) {
        int k = 0;
        while (k < kDpRuns && r.n[k]) {
            if (dst) { dst[2 * k] = r.lo[k]; dst[2 * k + 1] = r.n[k]; }
            ++k;
        }
        if (cnt) *cnt = k;
    };
    const DpRange o = dp_opt_range(&c, bk);
    put(o, own, out_nown);
    if (out_book) *out_book = o.book;
    put(dp_foreign_range(&c, bk), foreign, out_nforeign);
    return 0;
}

int vaeb_dw2_plan(const vaeb_config* cfg, int32_t* out_width, int32_t* out_paired, int32_t* out_workers,
                  int32_t* out_free_cus, int32_t* out_split, int32_t* ranges, int32_t cap) {
    if (!cfg) return fail(VAEB_ERR_ARG, "bad plan arguments");
    if (cfg->D <= 0 || cfg->H <= 0 || cfg->Z <= 0 || cfg->B <= 0) return fail(VAEB_ERR_ARG, "dimensions must be positive");
    // a host-only context (as vaeb_dp_plan): the same code the step and the flush run
    vaeb_ctx c;
    c.c = *cfg;
    set_arena_layout(&c);
    StepArgs a{};
    a.D = cfg->D; a.H = cfg->H; a.Z = cfg->Z;
    a.Mb = cfg->B; a.Mbp = r16(cfg->B);
    const int ct = enc_form(&c, a).ct;
    const W2Plan pl = w2_plan_for(&c, a);
    const int rows = a.H + 1, cols = (gaussian(&c) ? 2 : 1) * a.D, n = pl.tiles_i * pl.tiles_j;
    if (out_width) *out_width = pl.width;
    if (out_paired) *out_paired = pl.paired;
    if (out_workers) *out_workers = n;
    if (out_free_cus) *out_free_cus = kCUs - (a.Mbp / 16) * cdiv(a.H, 16 * ct);
    if (out_split) *out_split = gaussian(&c) ? a.D : 0;
    if (ranges) {
        if (cap < n) return fail(VAEB_ERR_ARG, "%d tile ranges do not fit %d", n, cap);
        for (int lt = 0; lt < n; ++lt) {   // wgrad_body's i0 / j0 of worker lt, clipped to the matrix
            const int i0 = (lt / pl.tiles_j) * kWT, j0 = (lt % pl.tiles_j) * pl.width;
            ranges[4 * lt] = i0;
            ranges[4 * lt + 1] = std::min(i0 + kWT, rows);
            ranges[4 * lt + 2] = j0;
            ranges[4 * lt + 3] = std::min(j0 + pl.width, cols);
        }
    }
    return 0;
}

}  // extern "C"

// vaeb_dp_rank_update's body, with the context's (world, rank, dp_shard) already set to the
// emulated rank's: the reduce-scatter's result uploaded, this rank's optimizer launch, the
// all-gather's result uploaded, the bf16 shadow fix -- dp_reduce_update with its collectives
// replaced by host copies, the kernels and index ranges unchanged.
static int dp_rank_update_body(vaeb_ctx* c, int bucket, const float* gsum, const float* thg) {
    const int par = c->par;
    hipStream_t s = c->s;
    const bool bf = is_bf16(c);
    const DpBucket bk = bucket == 0 ? dp_bucket_a_runs(c) : bucket == 1 ? dp_bucket_b_runs(c) : dp_bucket_all_runs(c);
    DpRange own = dp_opt_range(c, bk);
    own.book = 0;   // the SGVB bookkeeping (value, epoch sums, cursor, step) is not emulated
    const DpRange fr = dp_foreign_range(c, bk);
    // a step's first bucket (A, or all): the out arena -- theta' and the bf16 shadow -- NaN first,
    // so every element the step leaves there was written by it
    if (bucket != 1) {
        HIP_TRY(hipMemsetAsync(c->theta2[par ^ 1], 0xff, sizeof(float) * (size_t)c->P, s));
        if (bf) HIP_TRY(hipMemsetAsync(c->bf.shadow2[par ^ 1], 0xff, sizeof(bf16_t) * (size_t)c->bf.S, s));
    }
    // the reduce-scatter (+ all-reduce of the remainders): this rank's destinations hold the sum;
    // every other gradient element is NaN (the optimizer must not read it)
    HIP_TRY(hipMemsetAsync(c->grad, 0xff, sizeof(float) * (size_t)(c->P + 1), s));
    for (int k = 0; k < kDpRuns; ++k)
        if (own.n[k])
            HIP_TRY(hipMemcpyAsync(c->grad + own.lo[k], gsum + own.lo[k], sizeof(float) * (size_t)own.n[k],
                                   hipMemcpyHostToDevice, s));
    if (int rc = bf ? h16_dp_opt(c, par, own) : dp_opt_launch(c, s, make_opt(c, par, true, false), own, ElboArgs{}))
        return rc;
    if (thg) {
        // the all-gather: the other ranks' theta' shards into the out arena, then their shadow
        for (int k = 0; k < kDpRuns; ++k)
            if (fr.n[k])
                HIP_TRY(hipMemcpyAsync(c->theta2[par ^ 1] + fr.lo[k], thg + fr.lo[k], sizeof(float) * (size_t)fr.n[k],
                                       hipMemcpyHostToDevice, s));
        if (bf) if (int rc = h16_dp_fix(c, par, fr)) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

extern "C" {

int vaeb_dp_rank_update(vaeb_ctx* c, int32_t world, int32_t rank, int32_t bucket, const float* grad_sum,
                        int64_t n_grad, const float* theta_gathered, int32_t finish) {
    if (!c || !grad_sum || world <= 0 || world > 64 || rank < 0 || rank >= world || bucket < 0 || bucket > 2)
        return fail(VAEB_ERR_ARG, "bad dp_rank_update arguments");
    if (c->comm) return fail(VAEB_ERR_STATE, "vaeb_dp_rank_update emulates the collectives: use a context without a communicator");
    if (c->c.estimator == VAEB_EST_FV || c->c.estimator == VAEB_EST_FVS)
        return fail(VAEB_ERR_STATE, "the FV estimators have no data-parallel optimizer");
    if (n_grad != c->P + 1) return fail(VAEB_ERR_ARG, "size mismatch: got %lld, expected %lld", (long long)n_grad, (long long)(c->P + 1));
    if (int rc = w2_flush(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->s));
    const int w0 = c->world, r0 = c->rank;
    const bool s0 = c->dp_shard;
    c->world = world; c->rank = rank; c->dp_shard = world > 1;
    const int rc = dp_rank_update_body(c, bucket, grad_sum, theta_gathered);
    c->world = w0; c->rank = r0; c->dp_shard = s0;
    if (rc) return rc;
    if (finish) c->par ^= 1;
    return 0;
}

int vaeb_get_shadow(vaeb_ctx* c, uint16_t* out, int64_t n) {
    if (!c || !out) return fail(VAEB_ERR_ARG, "null argument");
    if (!is_bf16(c)) return fail(VAEB_ERR_STATE, "only the bf16 engine keeps a shadow arena");
    const int64_t nw = c->bf.smap.nweights;
    if (n != nw) return fail(VAEB_ERR_ARG, "size mismatch: got %lld, expected %lld", (long long)n, (long long)nw);
    if (int rc = w2_flush(c)) return rc;
    DevScratch scratch;   // freed on every return
    bf16_t* tmp = nullptr;
    if (int rc = scratch.alloc(&tmp, nw)) return rc;
    hipLaunchKernelGGL(bf::shadow_gather_kernel, dim3(1024), dim3(256), 0, c->s, (const bf16_t*)c->bf.shadow2[c->par], tmp,
                       c->bf.smap);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->s);
    if (e == hipSuccess) e = hipMemcpy(out, tmp, sizeof(bf16_t) * (size_t)nw, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(VAEB_ERR_HIP, "vaeb_get_shadow: %s", hipGetErrorString(e));
    return 0;
}

// The 16-bit step's buffers by name: a device pointer and its capacity in elements (include/vaeb_diag.h).
static int h16_copy_out(vaeb_ctx* c, const char* what, const char* name, const void* src, int64_t cap, size_t elem,
                        void* out, int64_t n) {
    if (!src) return fail(VAEB_ERR_STATE, "%s: buffer %s not allocated", what, name);
    if (n < 0 || n > cap)
        return fail(VAEB_ERR_ARG, "%s: buffer %s holds %lld elements, %lld requested", what, name, (long long)cap, (long long)n);
    HIP_TRY(hipStreamSynchronize(c->s));   // (a forked step has joined its second stream into c->s)
    HIP_TRY(hipMemcpy(out, src, elem * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

int vaeb_get_h16(vaeb_ctx* c, const char* name, uint16_t* out, int64_t n) {
    if (!c || !name || !out) return fail(VAEB_ERR_ARG, "null argument");
    if (!is_bf16(c)) return fail(VAEB_ERR_STATE, "vaeb_get_h16: only a 16-bit context keeps 16-bit step buffers");
    const bf::BfState& b = c->bf;
    const int64_t R = c->cap, RL = (int64_t)c->cap * c->c.L, H = c->c.H, Z = c->c.Z;
    const struct { const char* name; const uint16_t* p; int64_t cap; } bufs[] = {
        {"h", b.h, R * H}, {"z", b.z, RL * Z}, {"hd", b.hd, RL * H}, {"dA", b.dA, RL * b.Dn},
        {"dA1", b.dA1, RL * H}, {"dml", b.dml, R * 2 * Z}, {"dA3", b.dA3, R * H}};
    for (auto& e : bufs)
        if (strcmp(e.name, name) == 0) return h16_copy_out(c, "vaeb_get_h16", name, e.p, e.cap, sizeof(uint16_t), out, n);
    return fail(VAEB_ERR_ARG, "vaeb_get_h16: unknown buffer '%s'", name);
}

int vaeb_get_h16_f32(vaeb_ctx* c, const char* name, float* out, int64_t n) {
    if (!c || !name || !out) return fail(VAEB_ERR_ARG, "null argument");
    if (!is_bf16(c)) return fail(VAEB_ERR_STATE, "vaeb_get_h16_f32: only a 16-bit context keeps 16-bit step buffers");
    const bf::BfState& b = c->bf;
    const int64_t R = c->cap, RL = (int64_t)c->cap * c->c.L, Z = c->c.Z;
    const struct { const char* name; const float* p; int64_t cap; } bufs[] = {
        {"mu", b.mu, R * Z}, {"lv", b.lv, R * Z}, {"eps", b.eps, RL * Z}};
    for (auto& e : bufs)
        if (strcmp(e.name, name) == 0) return h16_copy_out(c, "vaeb_get_h16_f32", name, e.p, e.cap, sizeof(float), out, n);
    return fail(VAEB_ERR_ARG, "vaeb_get_h16_f32: unknown buffer '%s'", name);
}

int vaeb_kernel_name(int32_t id, char* out, int32_t cap) {
    if (!out || cap <= 0) return fail(VAEB_ERR_ARG, "bad buffer");
    const int n = (int)(sizeof(kKernelNames) / sizeof(kKernelNames[0]));
    if (id < 0 || id >= n) return fail(VAEB_ERR_ARG, "unknown kernel id %d", id);
    snprintf(out, (size_t)cap, "%s", kKernelNames[id]);
    return 0;
}

}  // extern "C"

// the layer-stack engine on the same fp32 tile engine: the host core of its handles, then the
// degenerate-vae autoencoder (vaeb_ae_*) and the softmax MLP classifier (vaeb_clf_*)
#include "stack_core.inc"
#include "engine_ae.inc"
#include "engine_clf.inc"
