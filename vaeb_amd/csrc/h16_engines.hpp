// h16_engines.hpp -- the 16-bit MFMA engine's device code, instantiated for both operand types:
//   namespace vaeb::bf  bf16 operands (v_mfma_f32_16x16x32_bf16)   VAEB_DTYPE_BF16
//   namespace vaeb::hf  fp16 operands (v_mfma_f32_16x16x32_f16)    VAEB_DTYPE_F16 (BASELINE config 5
//                       names "fp16 MFMA"; the same dense rate on gfx950)
// gemm_bf16.hpp, step_bf16.hpp and thin_bf16.hpp are written once against the names bf16_t /
// bf16x8 / f2bf / bf2f / mfma16 and included here twice; the element-type-independent part
// (BfState, ShadowMap, BatchRef) lives in h16_common.hpp.
#pragma once
#include <type_traits>
#include "tile_engine.hpp"
#include "kernels_aux.hpp"
#include "h16_common.hpp"

// fp16's range guard.  bf16 keeps fp32's exponent range; fp16's largest finite value is 65504,
// and a training step can leave it (a run from zero Adagrad accumulators at H = 2048 reaches
// |dLv| ~ 1e8 at its third step; a Gaussian decoder with log sigma^2 = -14 reaches |dA2| ~ 1e5).
// The fp16 instantiation therefore checks every value it converts for z, dA2 | dA6, dA1,
// [dMu | dLv] and dA3 and reports one outside +-65504 (or NaN / inf) in the control block's guard
// word (kernels_aux.hpp kStF16Range; gemm_bf16.hpp h16_report), which the step's ELBO reduction
// folds into the sticky status -> VAEB_ERR_NUMERIC.  Three macros carry it, so that the bf16
// instantiation compiles to exactly what it does without them:
//   H16_GUARD_FIELD   the guard word's address as the LAST member of an epilogue / argument struct
//                     (null: not a training step, nothing is reported)
//   H16_CHECK(bad, v) bad |= v is outside fp16's range
//   H16_REPORT(s, bad) report it to s.guard

#define VAEB_H16NS bf
#define VAEB_H16_F16 0
#define H16_GUARD_FIELD
#define H16_CHECK(bad, v) ((void)0)
#define H16_REPORT(s, bad) ((void)0)
#include "gemm_bf16.hpp"
#include "step_bf16.hpp"
#include "thin_bf16.hpp"
#undef VAEB_H16NS
#undef VAEB_H16_F16
#undef H16_GUARD_FIELD
#undef H16_CHECK
#undef H16_REPORT

#define VAEB_H16NS hf
#define VAEB_H16_F16 1
#define H16_GUARD_FIELD uint64_t* guard = nullptr;
#define H16_CHECK(bad, v) ((bad) |= !(__builtin_fabsf(v) <= 65504.f))
#define H16_REPORT(s, bad) h16_report((s).guard, (bad))
#include "gemm_bf16.hpp"
#include "step_bf16.hpp"
#include "thin_bf16.hpp"
#undef VAEB_H16NS
#undef VAEB_H16_F16
#undef H16_GUARD_FIELD
#undef H16_CHECK
#undef H16_REPORT
