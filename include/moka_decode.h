/*
 * moka_decode.h -- C ABI of the decode-step adapter kernel (libmoka_decode.so).
 *
 * After the prefill every generated token passes the adapted projections on the mask-free branch of the two reference layers
 *   AVT  AudioVisualText/peft_hyper/tuners/lora.py:373-381      VT  VisualText/modified_peft/tuners/lora/layer.py:672-678
 * which is plain LoRA with the text adapter:   y = x W^T + scale * (x A_text^T) B^T.
 * For the handful of tokens of such a step (T = batch x 1) the training forward of libmoka_hip.so (moka_down_fwd -> moka_up_fwd_fused ->
 * moka_weight_shadows, split-K slices and backward state through HBM) is launch-latency bound.  This library is the inference path:
 * ONE launch per group of projections that share their input, no workspace, no saved state, no interaction.  The frozen base GEMM
 * stays with the caller; the launch adds the adapter term in place onto its output.
 *
 * A library of its own: the contents of libmoka_hip.so / moka_hip.h are pinned (kernel forms, exported symbols, the source hash the
 * committed traffic summaries carry), and a decode step needs none of that library's state.  Conventions are those of moka_hip.h:
 * plain C symbols, raw device pointers + sizes + hipStream_t, 0 / negative MOKA_E* return codes, a thread-local message for the last
 * failure, everything enqueued on `stream`, no synchronisation, no allocation, no mutable state: the entry point captures into a
 * hipGraph as it is.
 */
#ifndef MOKA_DECODE_H
#define MOKA_DECODE_H

#include "moka_hip.h"            /* moka_stream_t, MOKA_BF16 / MOKA_F32, MOKA_E*, MOKA_MAX_GROUP */

#ifdef __cplusplus
extern "C" {
#endif

#define MOKA_DECODE_VERSION     100      /* 0.1.0 */
#define MOKA_DECODE_MAX_TOKENS  64       /* tokens of one call (batch x 1 of a cached decode step) */

int         moka_decode_version(void);
const char* moka_decode_last_error(void);
/* MOKA_DECODE_MAX_TOKENS */
int         moka_decode_max_tokens(void);

/* 1: moka_decode_fwd takes this call.  0: a valid shape the kernel does not serve -- fp32 storage (MOKA_F32), T < 1 or
 * T > moka_decode_max_tokens() -- the caller stays on the general path of libmoka_hip.so.  MOKA_EINVAL (< 0): arguments no path
 * accepts: G outside 1..MOKA_MAX_GROUP, r outside 1..64, a width that is not a positive multiple of 32, a null d_out, an unknown dtype. */
int         moka_decode_ok(int T, int d_in, const int* d_out /*[G]*/, int G, int r, int dtype);

/* y_g[t, :] += scale * (x[t, :] A_g^T) B_g^T   for g < G, t < T.
 *   x [T, d_in], A_g [r, d_in], B_g [d_out_g, r], y_g [T, d_out_g]: bf16, token-major, contiguous, every pointer 16-byte aligned
 *   (elements of the host pointer arrays included); 1 <= T <= moka_decode_max_tokens(), 1 <= G <= MOKA_MAX_GROUP, 1 <= r <= 64,
 *   d_in and d_out_g positive multiples of 32.  scale = s_in * s_out[text].
 * One launch.  Nothing else is read or written: rows >= T and rank rows >= r are neither stored nor read past their buffers.
 * Arithmetic: h = x A^T on v_mfma_f32_16x16x32_bf16 with fp32 accumulation (each workgroup computes all of h for its projection, its
 * waves split d_in and the partial sums are added through LDS in a fixed order), scale applied in fp32, h split into the bf16
 * hi + lo pair (hi + lo == h to 2^-17) that is multiplied with B, the sum added to y in fp32 and rounded to bf16 once.  No atomics:
 * a call is bitwise reproducible, a row's result does not depend on the other rows of the call, a projection's not on its group.
 * Arguments are checked on the host before anything is launched (MOKA_EINVAL, message in moka_decode_last_error()). */
int         moka_decode_fwd(const void* x, const void* const* A /*[G]*/, const void* const* Bw /*[G]*/, void* const* y_inout /*[G]*/,
                            const int* d_out /*[G]*/, int G, int T, int d_in, int r, float scale, moka_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MOKA_DECODE_H */
