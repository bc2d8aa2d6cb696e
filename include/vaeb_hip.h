/*
 * vaeb_hip.h -- C ABI of the MI355X-native VAEB SGVB training step (libvaeb_hip.so).
 *
 * The reference's operator boundary is the pair of Theano compiled functions built in
 * VAEB.getGradient (/root/reference/VAEB.py:408-422): `update(index) -> SGVB/B`
 * (mutating theta, the Adagrad accumulators and the RNG stream in place) and
 * `validate(x) -> SGVB` (forward-only sum).  This header exports those two operations
 * plus the state transfers the Python `VAEB` class needs (VAEB.py:132-242), as plain
 * `extern "C"` functions over host pointers and sizes.  No torch types appear here.
 *
 * Conventions
 *  - Every function returns int: 0 = ok, < 0 = error; vaeb_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - The caller owns host buffers (copied in/out during the call); the library owns all
 *    device memory.  One context per GPU/rank; calls on one context must be serialised.
 *  - Parameters are flat float32 in the reference order
 *    [W3,W4,W5,W1,W2,(W6),b3,b4,b5,b1,b2,(b6)] (VAEB.py:111-115), each row-major (C order).
 */
#ifndef VAEB_HIP_H
#define VAEB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum vaeb_decoder   { VAEB_DEC_BERNOULLI = 0, VAEB_DEC_GAUSSIAN = 1 };   /* --continuous, VAEB.py:256 */
enum vaeb_estimator { VAEB_EST_LB = 0, VAEB_EST_LA = 1, VAEB_EST_FV = 2,  /* VAEB.py:378-383 */
                      VAEB_EST_FVS = 3 };  /* extension (not in the reference code): full-variational
                                              with the weight-posterior reparameterisation that
                                              VAEB.sample_variational_params (VAEB.py:127-129)
                                              defines but never calls: theta~ = mu + |sigma| zeta */
enum vaeb_objective { VAEB_OBJ_SUM_PRIOR = 0,                             /* VAEB.py:386-390 */
                      VAEB_OBJ_MEAN_MAP = 1 };                            /* VAEBfullbayes.py:142,183 */
enum vaeb_eps_mode  { VAEB_EPS_PHILOX = 0, VAEB_EPS_HOST = 1 };
enum vaeb_dtype     { VAEB_DTYPE_F32 = 0,      /* fp32 MFMA, the reference's floatX (run_on_gpu.sh:2) */
                      VAEB_DTYPE_BF16 = 1,     /* bf16 MFMA operands, fp32 accumulation and fp32
                                                  master weights / Adagrad state (BASELINE config 5) */
                      VAEB_DTYPE_F16 = 2 };    /* fp16 MFMA operands ("fp16 MFMA", BASELINE config 5),
                                                  the same engine and fp32 state; the mean objective's
                                                  backward carries its 16-bit data gradients scaled by
                                                  a power of two ~ B_global (undone in fp32) */
enum vaeb_status    { VAEB_OK = 0, VAEB_ERR_ARG = -1, VAEB_ERR_HIP = -2, VAEB_ERR_STATE = -3,
                      VAEB_ERR_COMM = -4, VAEB_ERR_NOMEM = -5,
                      VAEB_ERR_NUMERIC = -6 };  /* a step's values left a range the engine depends on;
                                                   reported by the next vaeb_update /
                                                   vaeb_epoch_elbo, then cleared.  Either (fp32
                                                   engine) the fixed-point latent hand-off's range
                                                   (NaN / inf / |partial| >= 2^17): those latent
                                                   values were set to NaN; or (VAEB_DTYPE_F16) the
                                                   fp16 range: a training step stored z, dA2 | dA6,
                                                   dA1, [dMu | dLv] or dA3 outside +-65504 (or NaN /
                                                   inf) -- theta and the Adagrad state after that
                                                   step are not usable: restore them (vaeb_set_params,
                                                   vaeb_set_adagrad_state, a checkpoint) or train with
                                                   VAEB_DTYPE_BF16.  vaeb_last_error names which. */

typedef struct vaeb_config {
    int32_t D;            /* input size (784 MNIST, 560 Frey)                         */
    int32_t H;            /* hidden units (--hidden_unit, VAEB.py:542-552)             */
    int32_t Z;            /* latent size (--n_latent)                                  */
    int32_t B;            /* rows this rank processes per step                          */
    int32_t B_global;     /* rows of one global minibatch (= B * world for weak scaling) */
    int32_t row_offset;   /* first row of this rank inside the global minibatch          */
    int32_t L;            /* samples per datapoint (--L)                                 */
    int32_t decoder;      /* enum vaeb_decoder                                           */
    int32_t estimator;    /* enum vaeb_estimator                                         */
    int32_t objective;    /* enum vaeb_objective                                         */
    float   lr;           /* --learning_rate (VAEB.py:31)                                */
    float   adagrad_eps;  /* 1e-6 (VAEB.py:144)                                          */
    int32_t device;       /* HIP device ordinal                                          */
    int32_t max_eval_rows;/* largest x passed to vaeb_validate in one device chunk       */
    int32_t use_graph;    /* 1: replay the step as a captured hipGraph                   */
    int32_t keep_grads;   /* 1: also store each step's data gradient (vaeb_get_grads)    */
    int32_t dtype;        /* enum vaeb_dtype; BF16 needs D, H, Z % 8 == 0 (Gaussian: D % 32)  */
    int32_t reserved[5];
} vaeb_config;

typedef struct vaeb_ctx vaeb_ctx;

const char* vaeb_last_error(void);
int vaeb_version(int32_t* major, int32_t* minor);

/* Lifetime */
int vaeb_create(const vaeb_config* cfg, vaeb_ctx** out);
int vaeb_destroy(vaeb_ctx* ctx);
int vaeb_num_params(const vaeb_ctx* ctx, int64_t* n);

/* Training data: copied into a device-resident store owned by ctx (replaces the
 * th.shared x_train of VAEB.py:184).  Row-major float32 [n_rows x D].  16-bit contexts
 * keep it as fp16 / bf16 and, when every value is exactly 0 or 1 and D % 32 == 0, also as
 * bits (1/16 of that), from which the Bernoulli decoder expands its x tiles: the same
 * values, so the same steps bit for bit (one host pass over x decides). */
int vaeb_set_data(vaeb_ctx* ctx, const float* x, int64_t n_rows);

/* Parameters / optimizer state in reference order.  For the FV estimator the
 * "params" are the fixed data-term theta (VAEB.py:117-119) and the variational
 * (mu_theta, sigma_theta) pairs are transferred with vaeb_{set,get}_fv_state. */
int vaeb_set_params(vaeb_ctx* ctx, const float* flat, int64_t n);
int vaeb_get_params(vaeb_ctx* ctx, float* flat, int64_t n);
int vaeb_set_adagrad_state(vaeb_ctx* ctx, const float* flat, int64_t n);
int vaeb_get_adagrad_state(vaeb_ctx* ctx, float* flat, int64_t n);
/* FV: mu, sigma and their accumulators, each n = num_params floats. */
int vaeb_set_fv_state(vaeb_ctx* ctx, const float* mu, const float* sigma,
                      const float* acc_mu, const float* acc_sigma, int64_t n);
int vaeb_get_fv_state(vaeb_ctx* ctx, float* mu, float* sigma,
                      float* acc_mu, float* acc_sigma, int64_t n);

/* Noise for the reparameterisation (VAEB.py:41-47).  PHILOX: counter-based normals
 * keyed by (seed, step, global row, l, j), world-size invariant.  HOST: the caller
 * pushes eps [L x rows x Z] before each update/validate chunk (parity mode).
 *
 * The exact key (oracle/philox.py draws the same numbers on the host; tests/test_gpu_philox.py
 * compares).  One draw is Philox4x32-10 on a 128-bit counter (c0, c1, c2, c3) under the key
 * (low word of seed, high word of seed):
 *   c0      (uint32) row.  Training: batch_index * B_global + row_offset + m, m the row inside
 *           this rank's B.  vaeb_validate / vaeb_reconstruct_sampled / vaeb_marginal_ll: the
 *           row's index in the x passed to the call (not in the device chunk); the resident
 *           calls: the row's index in the resident set.
 *   c1      l * Z + j for sample l, latent j (evaluation streams: L of the context for
 *           vaeb_validate, one sample per stream otherwise, so c1 = j).
 *   c2, c3  low and high word of  step ^ (evaluation ? 1 << 63 : 0) ^ (stream << 40):
 *           stream 0 for training and validation, s for the s-th sample (1-based) of
 *           vaeb_reconstruct_sampled, k + 1 for importance sample k of vaeb_marginal_ll.
 *   eps = sqrt(-2 ln u1) cos(2 pi u2),  u1 = ((out0 >> 8) + 1) / 2^24,  u2 = (out1 >> 8) / 2^24.
 * VAEB_EST_FVS weight noise: parameter i (arena order) is normal i & 3 of group g = i >> 2 with
 * counter (uint32 g, 0x40000000 | g >> 32, step low, step high): r0 cos t0, r0 sin t0, r1 cos t1,
 * r1 sin t1, r from out0 / out2 and t from out1 / out3 as above.
 * Limits of this layout: rows are taken mod 2^32; L * Z < 2^30 (c1 bit 30 marks the weight
 * noise); the stream field occupies bits 40..62 of the step word, so streams and steps >= 2^40
 * overlap; hence n_samples, K <= 2^20.  Training steps draw at the counter and advance it by
 * one; evaluation calls draw at the current counter and leave it. */
int vaeb_set_eps_mode(vaeb_ctx* ctx, int32_t mode, uint64_t seed);
int vaeb_push_eps(vaeb_ctx* ctx, const float* eps, int64_t rows, int32_t L);
/* VAEB_EST_FVS in host eps mode: the standard normals zeta [P] (arena order) of the next
 * step's weight sample theta~ = mu + |sigma| zeta (Philox mode draws them on device). */
int vaeb_push_fv_noise(vaeb_ctx* ctx, const float* zeta, int64_t n);
int vaeb_set_step(vaeb_ctx* ctx, int64_t step);   /* Philox step counter */

/* One SGVB step on the contiguous minibatch `batch_index` (VAEB.py:413), synchronous
 * like the reference: writes SGVB / B_global to *out_elbo_per_row. */
int vaeb_update(vaeb_ctx* ctx, int32_t batch_index, float* out_elbo_per_row);
/* Throughput mode: enqueue one step, no host sync.  The ELBO stays on device and is
 * accumulated; read (and reset) the epoch mean with vaeb_epoch_elbo. */
int vaeb_update_async(vaeb_ctx* ctx, int32_t batch_index);
/* Enqueue a whole list of steps (an epoch's batch order) with one call. */
int vaeb_update_many(vaeb_ctx* ctx, const int32_t* batch_indices, int32_t n);
int vaeb_epoch_elbo(vaeb_ctx* ctx, double* out_sum, int64_t* out_steps);
int vaeb_synchronize(vaeb_ctx* ctx);

/* Forward-only SGVB sum over n rows of host x (VAEB.py:418-422). */
int vaeb_validate(vaeb_ctx* ctx, const float* x, int64_t n, double* out_sum);
/* Decoder means y for host x with z = mu (n_samples <= 0 branch of VAEB.reconstruct,
 * VAEB.py:267-270): writes [n x D]. */
int vaeb_reconstruct(vaeb_ctx* ctx, const float* x, int64_t n, float* out_y);
/* VAEB.reconstruct(x, n_samples) (VAEB.py:267-300): n_samples <= 0 as vaeb_reconstruct;
 * otherwise the decoder output averaged over n_samples posterior draws z = mu + exp(lv/2) eps
 * (Philox validation streams 1..n_samples, or in host eps mode rows [s*n, (s+1)*n) of the
 * pushed eps, which must hold n * n_samples rows).  Writes [n x D]. */
int vaeb_reconstruct_sampled(vaeb_ctx* ctx, const float* x, int64_t n, int32_t n_samples, float* out_y);
/* As vaeb_reconstruct_sampled, plus (Gaussian decoder, fp32 contexts; NULL to skip) the
 * decoder's log-sigma head hd W6 + b6 averaged over the same samples (VAEB.py:275-290): the
 * reference's closing draw is y + exp(out_lv) * N(0, 1) per pixel (VAEB.py:293-297). */
int vaeb_reconstruct_full(vaeb_ctx* ctx, const float* x, int64_t n, int32_t n_samples, float* out_y,
                          float* out_lv);
/* The decoder from given latents (freyFace.py:173-187 `image(z)`, compiled as `freyFace` at
 * :237-245): z [n x Z] -> mean [n x D] (sigmoid(tanh(z W1 + b1) W2 + b2)) and, for the Gaussian
 * decoder, the log-sigma head [n x D] (out_lv; NULL to skip).  fp32 contexts. */
int vaeb_decode(vaeb_ctx* ctx, const float* z, int64_t n, float* out_mu, float* out_lv);
/* Encoder outputs for host x [n x D]: mu and log-variance [n x Z] (VAEB.py:245-251).
 * Either output may be NULL.  fp32 contexts. */
int vaeb_encode(vaeb_ctx* ctx, const float* x, int64_t n, float* out_mu, float* out_lv);

/* Extension (no reference counterpart): the K-sample importance-weighted estimate of
 * sum_i log p(x_i), with the encoder as the proposal:
 *   z_k = mu(x) + exp(lv(x) / 2) eps_k,  log w_k = log p(x | z_k) + 1/2 sum_j (eps_kj^2 + lv_j - z_kj^2),
 *   IW_K(x) = logsumexp_k log w_k - log K    (IW_1: the one-sample LA estimate; rises to log p(x) with K).
 * out_sum: the sum over the n rows (double).  out_rows: per-row IW_K [n], or NULL.
 * Noise: Philox validation streams 1..K keyed by global row, exactly the streams
 * vaeb_reconstruct_sampled uses.  In host eps mode, rows [k*n, (k+1)*n) of the pushed
 * eps, which must hold n*K rows.  1 <= K <= 2^20.  The data term only (no thetaPrior), at the
 * current theta (VAEB_EST_FVS: the posterior mean); the context's L, estimator and objective
 * do not enter.  A non-finite log w makes that row's value and the sum NaN.  Changes no
 * training state.  fp32 contexts. */
int vaeb_marginal_ll(vaeb_ctx* ctx, const float* x, int64_t n, int32_t K,
                     double* out_sum, float* out_rows);
/* The same over the resident validation set (vaeb_set_valid_data): this rank's share of
 * the rows, all-reduced over the communicator like vaeb_validate_resident (host eps mode:
 * eps for nval*K rows, sample-major, global row order). */
int vaeb_marginal_ll_resident(vaeb_ctx* ctx, int32_t K, double* out_sum);

/* Data parallel (one ctx per rank): the library owns an RCCL communicator; the 128-byte
 * unique id is produced on rank 0 and broadcast by the host (e.g. torch.distributed). */
int vaeb_comm_unique_id(uint8_t out_id[128]);
int vaeb_comm_init(vaeb_ctx* ctx, const uint8_t id[128], int32_t rank, int32_t world);
/* Ranks in the context's communicator (ncclCommCount); 1 without a communicator. */
int vaeb_comm_count(vaeb_ctx* ctx, int32_t* out_world);

/* Device-resident validation set (VAEB.validate(x_valid) once per epoch, VAEB.py:582):
 * uploaded once; vaeb_validate_resident then evaluates this rank's contiguous share of
 * the rows (all rows without a communicator) with no host round trip between device
 * chunks and, with a communicator, all-reduces the SGVB sum over the ranks.  Noise rows
 * are keyed by the GLOBAL row (Philox), or read from the pushed eps (host mode: eps for
 * all n rows, global row order), so the result does not depend on the world size. */
int vaeb_set_valid_data(vaeb_ctx* ctx, const float* x, int64_t n_rows);
int vaeb_validate_resident(vaeb_ctx* ctx, double* out_sum);

/* Philox step counter (the number of noise draws so far), for checkpoints. */
int vaeb_get_step(vaeb_ctx* ctx, int64_t* step);

/* Native checkpoint (SURVEY 5 "checkpoint / resume"; the reference's VAEB.save keeps theta
 * only, VAEB.py:189-203, so a resumed run restarts Adagrad): one file holding the model
 * shape, theta, the Adagrad accumulators, the Philox seed / step and (FV / FVS) the
 * variational state.  A context loaded from it continues bit-identically to the run that
 * wrote it.  Loading checks that the file's D, H, Z, L, decoder and estimator match.
 * With a sharded data-parallel communicator (world > 1) saving is a collective: every rank
 * calls it (the Adagrad shards are all-gathered first); a rank passing path == NULL joins the
 * gather and writes nothing (rank 0 writes the file); NULL on a context without such a
 * communicator is VAEB_ERR_ARG. */
int vaeb_checkpoint_save(vaeb_ctx* ctx, const char* path);
int vaeb_checkpoint_load(vaeb_ctx* ctx, const char* path);

/* Introspection for parity tests: last step's data gradients (reference order, before
 * the prior) and named device activations ("h","mu","lv","z","hd","dA2","dA3",...). */
int vaeb_get_grads(vaeb_ctx* ctx, float* flat, int64_t n);
int vaeb_get_activation(vaeb_ctx* ctx, const char* name, float* out, int64_t n);

/* ------------------------------------------------------------------------------------------
 * degenerate-vae deterministic autoencoder (/root/reference/degenerate-vae/ae.py:41-117):
 * encoder MLP -> linear latent Z -> decoder MLP -> Bernoulli (otype "binary") or Gaussian
 * ("cont") output, logjoint = loglik + N(0, s2) prior on theta + N(0, 1) prior on Z, AdaGrad.
 * Parameters are flat float32 in the reference's theta order (ae.py:51,56,64,72):
 *   Wenc0..Wenc{n_enc-1}, benc0.., Wz, bz, Wdec0.., bdec0.., then Wout, bout (binary) or
 *   Wmu, Wlogs2, bmu, blogs2 (cont); W row-major [in x out].
 * ------------------------------------------------------------------------------------------ */
#define VAEB_AE_MAX_LAYERS 8
/* VAEB_AE_SE: the vanilla autoencoder's squared-error output (vanilla-ae/ae.py:63-72).  Sigmoid
 * output Xpr = sigmoid(Hx Wout + bout), theta tail [Wout, bout] as binary, se = sum (X - Xpr)^2 over
 * the step's rows, objective -se + N(0, s2) prior on theta (+ the latent's own term).
 * vaeb_ae_train / vaeb_ae_train_many write se / n: a POSITIVE error that falls as training
 * proceeds, while AdaGrad ascends -se (ae.py:72, 79).  Valid with the POINT latent (-se - 1/2 |Z|^2)
 * and the ACT latent; with GAUSS it is VAEB_ERR_ARG at create (-se is no log-likelihood, so the ELBO
 * and the importance-weighted bound have no meaning). */
enum vaeb_ae_otype { VAEB_AE_BINARY = 0, VAEB_AE_CONT = 1, VAEB_AE_SE = 2 };   /* ae.py:58 / :65 */
enum vaeb_act      { VAEB_ACT_TANH = 0, VAEB_ACT_SIGMOID = 1, VAEB_ACT_RELU = 2 };   /* f, ae.py:41 */
/* The latent layer.  POINT: the reference's degenerate VAE above.  GAUSS (extension: a deep VAE
 * on the same layer stack), on the rows X = Xtr[idx], M = |idx|, H the last encoder activation,
 * one sample per row:
 *   mu = H Wzmu + bzmu,  lv = H Wzlv + bzlv,  z = mu + exp(lv / 2) eps,  the decoder is fed z,
 *   negKL = 1/2 sum_{m,j} (1 + lv - mu^2 - exp(lv))     (replaces the N(0, 1) prior on Z),
 *   f = loglik + negKL + N(0, s2) prior on theta        (maximised by the same AdaGrad),
 * and train(idx) returns (loglik + negKL) / M.  In theta, [Wz, bz] become
 * [Wzmu, Wzlv, bzmu, bzlv] (the cont output's convention); everything else keeps its place.
 *
 * iw_samples = K >= 2 (GAUSS only; K on a POINT context, K < 0 or K > 2^20 is VAEB_ERR_ARG at
 * create; 0 and 1 are the ELBO step above, on its own code path): train on the K-sample
 * importance-weighted bound (Burda et al. 2016).  mu and lv once per row, then for k = 0..K-1
 *   z_k = mu + exp(lv / 2) eps_k,  log w_k = loglik_row(x | z_k) + 1/2 sum_j (eps_kj^2 + lv_j - z_kj^2)
 *   L_K = sum_m [logsumexp_k log w_mk - log K]           (vaeb_ae_marginal_ll's quantity)
 *   f   = L_K + N(0, s2) prior on theta,  train(idx) returns L_K / M,
 * with the reparameterised gradient sum_m sum_k wn_mk grad log w_mk - theta / s2,
 * wn_mk = w_mk / sum_k' w_mk' (no analytic KL enters).  The K sample planes are stacked in the
 * context's activation buffers, so a step needs K * M <= max_batch: otherwise VAEB_ERR_ARG before
 * the device is touched, with theta, the accumulators and the step unchanged.  A non-finite
 * log w_mk makes the step's value NaN (never dropped).  The evaluation calls behave exactly as on
 * an ELBO context.
 *
 * ACT (the vanilla autoencoder's code, vanilla-ae/ae.py:55): Z = f(H Wz + bz) with the context's
 * activation f and NO prior on Z; theta layout as POINT; valid with every otype.  vaeb_ae_encode
 * returns that Z, vaeb_ae_decode is unchanged.  The Gaussian-only calls below are VAEB_ERR_ARG, as
 * on POINT, and so is iw_samples >= 2.  Its value is 3: latent = 2 is unassigned and stays
 * VAEB_ERR_ARG at create, as every other unknown value (tests/test_vae_stack_host.py holds 2 to that). */
enum vaeb_ae_latent { VAEB_AE_LATENT_POINT = 0, VAEB_AE_LATENT_GAUSS = 1, VAEB_AE_LATENT_ACT = 3 };

typedef struct vaeb_ae_config {
    int32_t Dobs;                         /* observation size                                */
    int32_t n_enc;                        /* len(Denc) >= 1                                  */
    int32_t Denc[VAEB_AE_MAX_LAYERS];     /* encoder hidden sizes                            */
    int32_t Dz;                           /* latent size                                     */
    int32_t n_dec;                        /* len(Ddec) >= 1                                  */
    int32_t Ddec[VAEB_AE_MAX_LAYERS];     /* decoder hidden sizes                            */
    int32_t otype;                        /* enum vaeb_ae_otype                              */
    int32_t act;                          /* enum vaeb_act                                   */
    float   s2;                           /* prior variance on theta (ae.py:41, default 1.0) */
    float   eta;                          /* AdaGrad learning rate (infalg.py:144)           */
    int32_t max_batch;                    /* largest idx list / predict chunk                */
    int32_t device;
    int32_t latent;                       /* enum vaeb_ae_latent (0: the point latent)       */
    int32_t iw_samples;                   /* K of the training objective (below); 0, 1: ELBO */
    int32_t corruption;                   /* enum vaeb_ae_corruption (0: none), offset 112   */
    int32_t prior;                        /* enum vaeb_ae_prior (0: N(0, 1)), offset 116     */
} vaeb_ae_config;

typedef struct vaeb_ae vaeb_ae;

int vaeb_ae_create(const vaeb_ae_config* cfg, vaeb_ae** out);   /* ConstructAE (ae.py:41)    */
int vaeb_ae_destroy(vaeb_ae* ae);
int vaeb_ae_num_params(const vaeb_ae* ae, int64_t* n);
int vaeb_ae_set_data(vaeb_ae* ae, const float* x, int64_t n_rows);   /* Xtr (ae.py:87)        */
int vaeb_ae_set_params(vaeb_ae* ae, const float* flat, int64_t n);
int vaeb_ae_get_params(vaeb_ae* ae, float* flat, int64_t n);
int vaeb_ae_set_adagrad_state(vaeb_ae* ae, const float* flat, int64_t n);
int vaeb_ae_get_adagrad_state(vaeb_ae* ae, float* flat, int64_t n);
/* train(idx) (ae.py:82-89): one AdaGrad step on rows Xtr[idx]; writes loglik / n
 * (VAEB_AE_SE: se / n, positive). */
int vaeb_ae_train(vaeb_ae* ae, const int32_t* idx, int32_t n, float* out_loglik_per_row);
/* An epoch of train() calls on consecutive `batch`-sized slices of idx, the last partial
 * slice kept (ae.py:145-151); out[j] = train's value for slice j.  One host sync. */
int vaeb_ae_train_many(vaeb_ae* ae, const int32_t* idx, int32_t n, int32_t batch, float* out);
int vaeb_ae_reconstruct(vaeb_ae* ae, const float* x, int64_t n, float* out);   /* ae.py:92-98  */
int vaeb_ae_encode(vaeb_ae* ae, const float* x, int64_t n, float* z_out);      /* ae.py:101-107 */
int vaeb_ae_decode(vaeb_ae* ae, const float* z, int64_t n, float* out);        /* ae.py:110-116 */
/* Reconstruction error of host x [n x Dobs] on the device, on any context (every otype and latent):
 *   out_rows[i] = sum_d (x_id - Xpr_id)^2,  Xpr = vaeb_ae_reconstruct(x)
 * (Gaussian latent: z = mu; cont output: the mean head alone), out_rows may be NULL.  out_sum: the
 * sum of the row values (double, fixed order), so the vanilla autoencoder's mse()
 * (vanilla-ae/ae.py:120-121) is out_sum / n.  Runs in max_batch chunks; a row's value does not depend
 * on max_batch.  Changes no parameter, accumulator, step or pushed eps.  n <= 0 or a NULL x / out_sum
 * is VAEB_ERR_ARG before the device is touched. */
int vaeb_ae_sq_error(vaeb_ae* ae, const float* x, int64_t n, double* out_sum, float* out_rows);

/* VAEB_AE_LATENT_GAUSS contexts only (VAEB_ERR_ARG on a POINT or ACT context).  On such a
 * context vaeb_ae_encode returns mu, vaeb_ae_reconstruct decodes z = mu and vaeb_ae_decode is
 * unchanged.
 *
 * Noise, with the conventions of "Noise" above (enum vaeb_eps_mode; default PHILOX, seed 0,
 * step 0).  PHILOX: eps[m][j] is the draw at the counter (c0, c1 = j, c2, c3) under the seed:
 *   training    c0 = idx[m], the dataset row (so a row's draw does not depend on the batch it
 *               falls in); c2, c3 = the step.  Each train step draws at the context's step and
 *               advances it by one (vaeb_ae_train_many: one per slice).
 *   evaluation  (vaeb_ae_encode_dist's z, vaeb_ae_elbo) c0 = the row's index in the x passed to
 *               the call; c2, c3 = step ^ 1 << 63 (stream 0), at the current step, which stays.
 * HOST: the caller pushes eps [rows x Dz] in the row order of the next call (vaeb_ae_train_many:
 * of the whole idx list); a call that draws noise for another row count is VAEB_ERR_STATE.  The
 * pushed eps stays until the next push.
 * Training with iw_samples = K >= 2.  PHILOX: sample k of dataset row idx[m] is the draw at
 * c0 = idx[m], c1 = j, c2, c3 = the step with sample stream k (domain k << 1: the training domain),
 * so sample 0 is the ELBO context's draw for the same seed, row and step; each step advances the
 * step counter by one.  HOST: the push holds exactly K * n rows, n the length of the whole idx
 * list of the call, sample k of list position i at row k * n + i (VAEB_ERR_STATE otherwise). */
int vaeb_ae_set_eps_mode(vaeb_ae* ae, int32_t mode, uint64_t seed);
int vaeb_ae_push_eps(vaeb_ae* ae, const float* eps, int64_t rows);
int vaeb_ae_set_step(vaeb_ae* ae, int64_t step);    /* Philox step counter; these two also on any */
                                                    /* corrupting context (denoising training, below) */
int vaeb_ae_get_step(vaeb_ae* ae, int64_t* step);
/* Encoder outputs for host x [n x Dobs]: mu, log-variance and one evaluation-noise sample
 * z = mu + exp(lv / 2) eps, each [n x Dz]; any of the three may be NULL (no noise is drawn
 * without out_z). */
int vaeb_ae_encode_dist(vaeb_ae* ae, const float* x, int64_t n, float* out_mu, float* out_lv, float* out_z);
/* Forward-only sum of loglik + negKL over n rows of host x with evaluation noise, in max_batch
 * chunks (no theta prior).  Changes no parameter, accumulator or step. */
int vaeb_ae_elbo(vaeb_ae* ae, const float* x, int64_t n, double* out_sum);
/* The K-sample importance-weighted estimate of sum_i log p(x_i) for host x [n x Dobs], with the
 * encoder as the proposal (vaeb_marginal_ll's quantity on the layer stack).  Per row, mu and lv
 * are computed once, then for k = 0..K-1
 *   z_k = mu + exp(lv / 2) eps_k,  log w_k = loglik_row(x | z_k) + 1/2 sum_j (eps_kj^2 + lv_j - z_kj^2),
 *   IW_K(x) = logsumexp_k log w_k - log K,
 * loglik_row being the output layer above (binary: the 1e-7 inside the logs); no theta prior and
 * no analytic KL enter.  out_sum: the sum of the row values (double, fixed order).  out_rows:
 * IW_K per row [n], or NULL.  1 <= K <= 2^20, else VAEB_ERR_ARG before the device is touched.
 * Noise.  PHILOX: sample k draws from evaluation stream k + 1 (domain 1 | (k + 1) << 1): c0 = the
 * row's index in the x passed to the call, c1 = j, c2, c3 from the current step, which stays.
 * HOST: the pushed eps must hold exactly n * K rows, sample k of row i at row k * n + i
 * (VAEB_ERR_STATE otherwise), and stays.
 * A non-finite log w_k makes that row's value and *out_sum NaN (never dropped); other rows are
 * unaffected.  A row's value does not depend on max_batch.  Changes no parameter, accumulator,
 * step or pushed eps.  Device memory does not grow with K or n (scratch sized by max_batch,
 * allocated on the first call). */
int vaeb_ae_marginal_ll(vaeb_ae* ae, const float* x, int64_t n, int32_t K, double* out_sum, float* out_rows);

/* Denoising training (extension): vaeb_ae_config.corruption != VAEB_AE_CORRUPT_NONE.  A training
 * step on the rows idx (M rows, X = Xtr[idx]) first forms xt [M x Dobs] from X and the context's
 * noise level p:
 *   MASK         xt = 0 if r < p, else x
 *   SALT_PEPPER  xt = 0 if r < p / 2;  1 if p / 2 <= r < p;  else x
 *   GAUSS        xt = x + p n
 * r a uniform in [0, 1) on the 2^-24 grid, n a standard normal, one draw per element (m, d).  The
 * comparisons are float32 comparisons of exactly representable values (p / 2 is exact).  The
 * encoder's first layer reads xt, in the forward and in its weight and bias gradient; everything
 * that scores or reports against the data keeps the clean X: the output layer's observations (every
 * otype, and each sample plane with iw_samples >= 2) and the returned value, which is
 * loglik(X | enc(xt)) / M, (loglik - KL) / M, L_K / M or se / M.  The value and its gradient are
 * those of the context's objective with the encoder's input replaced by xt; no other term
 * appears.  This is the denoising autoencoder (POINT, ACT) and the denoising VAE (GAUSS latent);
 * a schedule of falling levels is vaeb_ae_set_corruption_level between calls.  Valid with every
 * latent, every otype and iw_samples >= 2 (one corruption per dataset row, shared by its K
 * samples: the encoder runs once per row).  The evaluation calls (vaeb_ae_reconstruct, _encode,
 * _decode, _encode_dist, _elbo, _marginal_ll, _sq_error) never corrupt: to denoise a row, pass
 * the corrupted row to vaeb_ae_reconstruct.  Any other value of `corruption` is VAEB_ERR_ARG at
 * create, before the device is touched.
 *
 * Noise, with the conventions of "Noise" above and a mode and seed of its own (default PHILOX,
 * seed 0); vaeb_ae_set_eps_mode stays a Gaussian-latent call.  PHILOX: one Philox4x32-10 block per
 * element under the key (seed lo, seed hi) at the counter
 *   c0      idx[m], the dataset row: a row's corruption depends neither on the batch nor on the
 *           position it falls in, and a row repeated in one idx list is corrupted identically
 *   c1      0x80000000 | d.  Bit 31 marks input corruption (the latent draws have c1 < 2^30, the
 *           FVS weight noise sets bit 30), so Dobs < 2^30 and the layout is disjoint from every
 *           other draw
 *   c2, c3  the training domain at the context's step counter (step, stream 0)
 *   r = (out2 >> 8) / 2^24;  n = sqrt(-2 ln u1) cos(2 pi u2) on out0 and out1, as eps above.
 * HOST: the caller pushes a float matrix [rows x Dobs] (r values for MASK and SALT_PEPPER, n values
 * for GAUSS) in the order of the next training call's whole idx list, one row per list position,
 * also with iw_samples >= 2; a training call of another row count is VAEB_ERR_STATE before the
 * device is touched.  The push stays until the next push.
 * The step counter: on a corrupting context every training step advances it by one, whatever the
 * latent (a Gaussian-latent context still once per step: its latent and corruption draws of one
 * step share the step word), and vaeb_ae_set_step / vaeb_ae_get_step are accepted.
 * Limits: Dobs < 2^30 and max_batch * Dobs < 2^29 (VAEB_ERR_ARG at create).
 * The five calls below are VAEB_ERR_ARG on a context created with VAEB_AE_CORRUPT_NONE. */
enum vaeb_ae_corruption { VAEB_AE_CORRUPT_NONE = 0, VAEB_AE_CORRUPT_MASK = 1, VAEB_AE_CORRUPT_SALT_PEPPER = 2,
                          VAEB_AE_CORRUPT_GAUSS = 3 };
/* The level p: 0 after create.  MASK and SALT_PEPPER: 0 <= level <= 1; GAUSS: level >= 0 and
 * finite; NaN or out of range is VAEB_ERR_ARG with the level unchanged.  The level is passed to
 * the launches by value: no synchronise, and steps already enqueued keep theirs. */
int vaeb_ae_set_corruption_level(vaeb_ae* ae, float level);
int vaeb_ae_get_corruption_level(vaeb_ae* ae, float* out_level);
/* mode: VAEB_EPS_PHILOX or VAEB_EPS_HOST. */
int vaeb_ae_set_corruption_noise(vaeb_ae* ae, int32_t mode, uint64_t seed);
int vaeb_ae_push_corruption(vaeb_ae* ae, const float* r, int64_t rows);
/* The xt [n x Dobs] a training call on idx would read at the current step, level and mode (HOST:
 * the pushed rows, which must number n).  Changes no parameter, accumulator, step or push; runs in
 * max_batch chunks, so n need not fit max_batch. */
int vaeb_ae_corrupt(vaeb_ae* ae, const int32_t* idx, int32_t n, float* out);

/* Two-mode latent prior and binary codes (extension): vaeb_ae_config.prior == VAEB_AE_PRIOR_TWO_MODE,
 * VAEB_AE_LATENT_GAUSS contexts only.  Per latent dimension the N(0, 1) prior is replaced by an
 * equal-weight mixture of two Gaussians of one width,
 *   p(z) = 1/2 N(z; 0, s^2) + 1/2 N(z; a, s^2),      a = mean1, s = width, c = 1 / s^2,
 * which pulls every latent towards {0, a}: a sparsity-inducing prior under which a row is encoded
 * as Dz bits by truncating the posterior mean.  Per element (row m, latent j):
 *   t = a (2 z - a) c / 2,   r = sigmoid(t)          (the responsibility of the mode at a)
 *   log p(z) = -1/2 log 2 pi - log(2 s) - 1/2 c z^2 + softplus(t),   dlog p / dz = -c (z - a r),
 * softplus(t) = max(t, 0) + log(1 + exp(-|t|)) (t reaches 1e3 at small widths).
 * The ELBO step (iw_samples 0 or 1).  The KL to a mixture has no closed form, so the prior term is
 * taken at the step's sample z = mu + exp(lv / 2) eps and the entropy stays analytic:
 *   latent_row = sum_j [1/2 (1 + lv_j) - log(2 s) - 1/2 c z_j^2 + softplus(t_j)]   (replaces negKL)
 *   train(idx) returns (loglik + sum_m latent_row) / M,  and with dz the decoder's gradient into z
 *   g = dz - c (z - a r),   dmu = g,   dlv = 1/2 g (z - mu) + 1/2.
 * vaeb_ae_elbo sums loglik + latent_row with evaluation noise.
 * The importance-weighted forms (vaeb_ae_marginal_ll on such a context; training with iw_samples >= 2):
 *   log w_k = loglik_row(x | z_k) + sum_j [1/2 eps_kj^2 + 1/2 lv_j - log(2 s) - 1/2 c z_kj^2 + softplus(t_kj)]
 *   u = dz - wn c (z - a r),   dmu_k = u,   dlv_k = 1/2 u (z - mu) + 1/2 wn.
 * At a = 0, s = 1 the importance-weighted forms are the N(0, 1) context's 1/2 sum (eps^2 + lv - z^2)
 * and u = dz - wn z (equal up to rounding: the arithmetic differs); the ELBO form is then a
 * one-sample estimate whose expectation over eps is the analytic negKL, not the same number per step.
 * Nothing else changes: the theta layout, the noise draws, the Philox keys and the step counter are
 * those of the N(0, 1) context, as are vaeb_ae_encode, _reconstruct, _decode, _encode_dist and
 * _sq_error.  Valid with every otype a GAUSS context allows, with iw_samples >= 2 and with every
 * corruption.  Any other value of `prior`, or TWO_MODE on a POINT or ACT context, is VAEB_ERR_ARG at
 * create, before the device is touched.  A context of the N(0, 1) prior launches what it launched
 * before the extension existed.
 * The four calls below are VAEB_ERR_ARG on a context created with VAEB_AE_PRIOR_NORMAL. */
enum vaeb_ae_prior { VAEB_AE_PRIOR_NORMAL = 0, VAEB_AE_PRIOR_TWO_MODE = 1 };
/* mean1 = 1 and width = 0.25 after create.  Valid: finite |mean1| <= 1e3 and 1e-3 <= width <= 1e3
 * (c and t stay finite in float32 for any sane z); NaN or out of range is VAEB_ERR_ARG with both
 * values unchanged.  a, c and log(2 s) are passed to the launches by value: no synchronise, and
 * steps already enqueued keep theirs.  A schedule of falling widths is vaeb_ae_set_prior between
 * training calls. */
int vaeb_ae_set_prior(vaeb_ae* ae, float mean1, float width);
int vaeb_ae_get_prior(vaeb_ae* ae, float* mean1, float* width);
/* Binary codes.  encode_bits: bit j of row i is mu_ij >= a / 2 (mu = vaeb_ae_encode's output, a
 * float32 comparison), packed into out_words [n x ceil(Dz / 32)]: bit j at word j / 32, bit j % 32;
 * the padding bits of a row's last word are 0.  decode_bits: vaeb_ae_decode of z_ij = a where the
 * bit is set, else 0; out [n x Dobs].  Both run in max_batch chunks (n need not fit max_batch) and
 * change no parameter, accumulator, step or push.  n <= 0 or a NULL pointer is VAEB_ERR_ARG before
 * the device is touched. */
int vaeb_ae_encode_bits(vaeb_ae* ae, const float* x, int64_t n, uint32_t* out_words);
int vaeb_ae_decode_bits(vaeb_ae* ae, const uint32_t* words, int64_t n, float* out);

/* The update rule of the layer-stack engine (extension beyond AdaGrad; the reference's other two
 * optimisers, infalg.py:44-137, and Adam).  Every rule ASCENDS f with g = df/dtheta (the prior's
 * -theta / s2 included) in the weight-gradient launch's epilogue; a step launches the same kernels
 * in the same order whatever the rule.  Per element, with state slots s0 and s1 laid out as theta:
 *   ADAGRAD   s0' = s0 + g^2;  theta += eta g / (sqrt(s0') + 1e-6)
 *   SGA       s0' = beta1 s0 + g;  theta += eta s0'          (beta1: the momentum mu in [0, 1);
 *             at mu = 0 slot 0 after a step IS that step's gradient)
 *   ADADELTA  s0' = rho s0 + (1 - rho) g^2;  dx = sqrt(s1 + eps) g / sqrt(s0' + eps);
 *             theta += eta dx;  s1' = rho s1 + (1 - rho) dx^2   (beta1: rho in (0, 1); s0 = g_ac,
 *             s1 = dx_ac; eta = 1 is the reference's rule)
 *   ADAM      s0' = beta1 s0 + (1 - beta1) g;  s1' = beta2 s1 + (1 - beta2) g^2;
 *             theta += eta (s0' / (1 - beta1^t)) / (sqrt(s1' / (1 - beta2^t)) + eps)
 *             (t: the optimiser step counter below after this step, 1 for the first)
 * A fresh context is {ADAGRAD, cfg.eta, 0, 0, 1e-6} and steps exactly as it did before this call
 * existed.  vaeb_ae_set_optimizer with ANOTHER rule zeroes both slots and the step counter (on the
 * context's stream, after the steps already enqueued); with the SAME rule it changes the
 * hyper-parameters only -- a step-size schedule between train calls, for AdaGrad too.  They are
 * launch arguments: steps already enqueued keep theirs.  VAEB_ERR_ARG: an unknown rule; eta <= 0;
 * a beta outside [0, 1) (rho outside (0, 1)); eps <= 0 for ADADELTA / ADAM; ADAGRAD with eps other
 * than 1e-6f (its kernel keeps the literal); a field the rule does not use set non-zero (ADAGRAD:
 * beta1, beta2; SGA: beta2, eps; ADADELTA: beta2).
 * State: slot 0 is also vaeb_ae_set / get_adagrad_state's array; slot 1 exists for ADADELTA and
 * ADAM only (VAEB_ERR_ARG otherwise, as n != num_params).  The optimiser step counter advances by
 * one per training step under every rule; it is not the Philox step counter. */
enum vaeb_ae_rule { VAEB_AE_RULE_ADAGRAD = 0, VAEB_AE_RULE_SGA = 1, VAEB_AE_RULE_ADADELTA = 2, VAEB_AE_RULE_ADAM = 3 };
typedef struct vaeb_ae_optimizer {
    int32_t rule;                         /* enum vaeb_ae_rule                               */
    float eta, beta1, beta2, eps;
} vaeb_ae_optimizer;                      /* 20 bytes                                        */
int vaeb_ae_set_optimizer(vaeb_ae* ae, const vaeb_ae_optimizer* opt);
int vaeb_ae_get_optimizer(vaeb_ae* ae, vaeb_ae_optimizer* out);
int vaeb_ae_set_opt_state(vaeb_ae* ae, int32_t slot, const float* flat, int64_t n);
int vaeb_ae_get_opt_state(vaeb_ae* ae, int32_t slot, float* flat, int64_t n);
int vaeb_ae_set_opt_step(vaeb_ae* ae, int64_t t);
int vaeb_ae_get_opt_step(vaeb_ae* ae, int64_t* t);

/* ------------------------------------------------------------------------------------------
 * Softmax MLP classifier on the layer stack (the reference's degenerate-vae/mlp.py:104-153 the MAP
 * classifier, :263-329 the dropout one, :332-388 its learning loop): hidden layers
 * H_{i+1} = f(H_i W_i + b_i), H_0 = X, logits a = H_n Wout + bout, P = softmax(a) (logpdf.py:16-17).
 * Targets Y are a float matrix [n x Dout] in [0, 1] (1-hot in the reference), not class indices.
 * Per row, with e = exp(a - max a) and P = e / sum e:
 *   VAEB_CLF_BERNOULLI    ll = sum_j Y_j log(P_j + 1e-7) + (1 - Y_j) log(1 - P_j + 1e-7)   (mlp.py:112),
 *                         dll/da_i = P_i (dP_i - sum_j P_j dP_j),
 *                         dP_j = Y_j / (P_j + 1e-7) - (1 - Y_j) / (1 - P_j + 1e-7)
 *   VAEB_CLF_CATEGORICAL  (extension) ll = sum_j Y_j (a_j - max a - log sum e),  dll/da_i = Y_i - P_i sum_j Y_j
 * The objective f of a step on M rows is the SUM of the rows' ll, plus with prior = 1 the N(0, s2)
 * prior on theta (gradient - theta / s2); prior = 0 is the reference ("logjoint = loglik #+ logprior").
 * Every update rule of vaeb_ae_optimizer ascends f; a fresh context is {ADAGRAD, cfg.eta, 0, 0, 1e-6}.
 * Theta is flat float32 in the reference's order (mlp.py:113, 277): W0..W{n-1}, b0..b{n-1}, Wout,
 * bout; W row-major [in x out].
 *
 * Weight dropout (dropout = 1; mlp.py:265-277 at keep = 0.5): every call of the network uses
 * theta~ = theta * m with a fresh m ~ Bernoulli(keep) per PARAMETER (weights and biases alike).  A
 * training step draws m, runs the forward and the data backward on theta~, and applies the rule to
 * the real theta with g = m * (the weight gradient) - theta / s2: a dropped parameter sees the
 * prior's pull alone (0 without a prior), and the rule does with that whatever it does.
 * The draw: parameter i of the flat arena takes output word i & 3 of the Philox4x32-10 block at
 *   c0 = i >> 2,  c1 = 0x40000000 (a site of its own: the latent draws have c1 < 2^30, the input
 *   corruption sets bit 31),  c2, c3 = the step word of "Noise" above: domain 0 at the context's
 *   step counter for training, domain 1 | (l + 1) << 1 for evaluation draw l,
 * under the key (seed lo, seed hi), and is kept iff word < T, T = floor(keep * 2^32) computed once
 * in double from the float32 keep (so the kept fraction is T / 2^32 <= keep, below it by less than
 * 2^-32; keep = 1 gives T = 2^32 and keeps every parameter: such a context steps bit for bit as
 * a dropout = 0 context).  The step counter advances by one per training step on EVERY context, so
 * a schedule means the same on a MAP and a dropout context; evaluation calls leave it.
 *
 * Every bad argument is VAEB_ERR_ARG before the device is touched, with the state unchanged: at
 * create Din <= 0, n_hidden outside 1..VAEB_AE_MAX_LAYERS, a Dh <= 0, Dout < 2, an unknown act /
 * loss / prior / dropout, prior = 1 without a finite s2 > 0, eta not finite and > 0, max_batch <= 0,
 * dropout = 1 with keep outside (0, 1] or not finite. */
enum vaeb_clf_loss { VAEB_CLF_BERNOULLI = 0, VAEB_CLF_CATEGORICAL = 1 };
typedef struct vaeb_clf_config {
    int32_t Din;                          /* input size                                       */
    int32_t n_hidden;                     /* len(Dh), 1..VAEB_AE_MAX_LAYERS                   */
    int32_t Dh[VAEB_AE_MAX_LAYERS];       /* hidden sizes                                     */
    int32_t Dout;                         /* classes, >= 2 (offset 40)                        */
    int32_t act;                          /* enum vaeb_act                                    */
    int32_t loss;                         /* enum vaeb_clf_loss                               */
    int32_t prior;                        /* 0: none (the reference); 1: N(0, s2) on theta    */
    float   s2;                           /* prior variance (read with prior = 1)             */
    float   eta;                          /* AdaGrad step size of the rule in force at create */
    int32_t max_batch;                    /* largest training batch / evaluation chunk        */
    int32_t device;
    int32_t dropout;                      /* 0: MAP classifier; 1: weight dropout (offset 72) */
    float   keep;                         /* Bernoulli keep probability (read with dropout = 1) */
} vaeb_clf_config;                        /* 80 bytes                                         */

typedef struct vaeb_clf vaeb_clf;

int vaeb_clf_create(const vaeb_clf_config* cfg, vaeb_clf** out);
int vaeb_clf_destroy(vaeb_clf* clf);
int vaeb_clf_num_params(const vaeb_clf* clf, int64_t* n);
/* Xtr [n_rows x Din] and Ytr [n_rows x Dout], both copied to the device. */
int vaeb_clf_set_data(vaeb_clf* clf, const float* x, const float* y, int64_t n_rows);
int vaeb_clf_set_params(vaeb_clf* clf, const float* flat, int64_t n);
int vaeb_clf_get_params(vaeb_clf* clf, float* flat, int64_t n);
/* The update rule and its state: the semantics and argument checks of the vaeb_ae_* calls of the
 * same names (slot 0 is AdaGrad's accumulator; under SGA at momentum 0 it holds the last step's
 * gradient g). */
int vaeb_clf_set_optimizer(vaeb_clf* clf, const vaeb_ae_optimizer* opt);
int vaeb_clf_get_optimizer(vaeb_clf* clf, vaeb_ae_optimizer* out);
int vaeb_clf_set_opt_state(vaeb_clf* clf, int32_t slot, const float* flat, int64_t n);
int vaeb_clf_get_opt_state(vaeb_clf* clf, int32_t slot, float* flat, int64_t n);
int vaeb_clf_set_opt_step(vaeb_clf* clf, int64_t t);
int vaeb_clf_get_opt_step(vaeb_clf* clf, int64_t* t);
/* The dropout draws' Philox key and step counter (seed 0, step 0 after create); accepted on any
 * context. */
int vaeb_clf_set_seed(vaeb_clf* clf, uint64_t seed);
int vaeb_clf_set_step(vaeb_clf* clf, int64_t step);
int vaeb_clf_get_step(vaeb_clf* clf, int64_t* step);
/* One step on the rows idx [n] of the resident data (n <= max_batch, every index in range, else
 * VAEB_ERR_ARG); writes the step's log-likelihood SUM (the reference's outputs=logjoint): the
 * fixed-order fp64 sum of the row values, stored as float.  train_many: consecutive batch-sized
 * slices of idx, the last partial slice kept, out[j] the value of slice j, one host sync. */
int vaeb_clf_train(vaeb_clf* clf, const int32_t* idx, int32_t n, float* out_loglik_sum);
int vaeb_clf_train_many(vaeb_clf* clf, const int32_t* idx, int32_t n, int32_t batch, float* out);
/* The evaluation calls take host rows, run in max_batch chunks (n need not fit max_batch) and
 * change no parameter, optimiser state or step.  `draws` = 0 (`draw` = -1) uses theta as it is;
 * draws = L >= 1 (L <= 2^20) is valid on dropout contexts only and averages softmax under theta~
 * over the evaluation draws 0..L-1, accumulated on the device; draw >= 0 uses that one evaluation
 * draw.  Equal calls return equal bits.
 * predict: P [n x Dout].  loglik: the fp64 sum over the rows of ll (no prior).  accuracy: the
 * number of rows with y[i][argmax_j P_ij] == 1 (mlp.py:367-373; the lowest index among equal P, as
 * numpy.argmax), counted on the device in integers. */
int vaeb_clf_predict(vaeb_clf* clf, const float* x, int64_t n, int32_t draws, float* out);
int vaeb_clf_loglik(vaeb_clf* clf, const float* x, const float* y, int64_t n, int32_t draw, double* out_sum);
int vaeb_clf_accuracy(vaeb_clf* clf, const float* x, const float* y, int64_t n, int32_t draws, int64_t* correct);
/* The byte mask m [num_params] (1 kept, 0 dropped) of the training step at `step` (draw = -1) or of
 * evaluation draw `draw` >= 0 at `step`; dropout contexts only.  Changes no state. */
int vaeb_clf_draw_mask(vaeb_clf* clf, int64_t step, int32_t draw, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* VAEB_HIP_H */
