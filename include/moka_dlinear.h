/*
 * moka_dlinear.h -- C ABI of the decode-step adapted projection (libmoka_dlinear.so): base GEMV with the adapter fused.
 *
 * A cached decode step passes every adapted projection on the mask-free branch of the two reference layers (see moka_decode.h):
 *   y = x W^T (+ bias) + scale * (x A_text^T) B^T
 * libmoka_decode.so leaves the frozen base GEMM with the caller and adds the adapter term onto its bf16 output -- y is rounded twice and
 * crosses HBM three times.  For T = batch x 1 <= 16 tokens the base is a weight-streaming GEMV (W is read once, nothing else counts),
 * and this library owns it: ONE launch per group of projections that share their input computes base, bias and adapter term in fp32 and
 * rounds y once.  No second copy of the projection weights (MokaLlamaStack.merge_for_decode), the adapters stay separate.
 *
 * A library of its own for the reasons moka_decode.h gives: the contents of libmoka_hip.so and of libmoka_decode.so are pinned.
 * Conventions are theirs: plain C symbols, raw device pointers + sizes + hipStream_t, 0 / negative MOKA_E* return codes, a thread-local
 * message for the last failure, everything enqueued on `stream`, no workspace, no synchronisation, no allocation, no mutable state: the
 * entry point captures into a hipGraph as it is.
 */
#ifndef MOKA_DLINEAR_H
#define MOKA_DLINEAR_H

#include "moka_hip.h"            /* moka_stream_t, MOKA_BF16 / MOKA_F32, MOKA_E*, MOKA_MAX_GROUP */

#ifdef __cplusplus
extern "C" {
#endif

#define MOKA_DLINEAR_VERSION     100      /* 0.1.0 */
#define MOKA_DLINEAR_MAX_TOKENS  16       /* tokens of one call: one MFMA token tile (above it the base belongs to hipBLASLt) */

int         moka_dlinear_version(void);
const char* moka_dlinear_last_error(void);
/* MOKA_DLINEAR_MAX_TOKENS */
int         moka_dlinear_max_tokens(void);

/* 1: moka_dlinear_fwd takes this call.  0: a valid shape the kernel does not serve -- fp32 storage (MOKA_F32), T < 1 or
 * T > moka_dlinear_max_tokens() -- the caller stays on the paths of libmoka_decode.so / libmoka_hip.so.  MOKA_EINVAL (< 0): arguments
 * no path accepts: G outside 1..MOKA_MAX_GROUP, r outside 1..64, a width that is not a positive multiple of 32, a null d_out, an
 * unknown dtype. */
int         moka_dlinear_ok(int T, int d_in, const int* d_out /*[G]*/, int G, int r, int dtype);

/* y_g[t, :] = bf16( x[t, :] W_g^T + bias_g + scale * (x[t, :] A_g^T) B_g^T )   for g < G, t < T.
 *   x [T, d_in], W_g [d_out_g, d_in] (row-major, as nn.Linear.weight stores it), bias_g [d_out_g], A_g [r, d_in], B_g [d_out_g, r],
 *   y_g [T, d_out_g]: bf16, contiguous, every pointer 16-byte aligned (elements of the host pointer arrays included);
 *   `bias` is NULL (no projection has one) or an array of G entries of which any may be NULL;
 *   1 <= T <= moka_dlinear_max_tokens(), 1 <= G <= MOKA_MAX_GROUP, 1 <= r <= 64, d_in and d_out_g positive multiples of 32.
 *   scale = s_in * s_out[text].
 * One launch.  y is WRITTEN, never read; nothing else is written: rows >= T are not stored, and nothing is read past a buffer.
 * Arithmetic: a workgroup owns a block of output columns of one projection and reads its rows of W once; the base product and
 * h = x A^T come from the same pass over d_in on v_mfma_f32_16x16x32_bf16 with fp32 accumulation (the waves split d_in, their partial
 * sums are added through LDS in a fixed order that depends on neither T, G nor the column block); h is scaled in fp32 and split into
 * the bf16 hi + lo pair (hi + lo == h to 2^-17) that is multiplied with B ONTO the fp32 base sums; the bias is added in fp32 and the
 * result rounded to bf16 once.  No atomics and no hand-over between workgroups: a call is bitwise reproducible, a row's result does
 * not depend on the other rows of the call, a projection's not on its group.
 * Arguments are checked on the host before anything is launched (MOKA_EINVAL, message in moka_dlinear_last_error()). */
int         moka_dlinear_fwd(const void* x, const void* const* W /*[G]*/, const void* const* bias /* NULL or [G], entries may be NULL */,
                             const void* const* A /*[G]*/, const void* const* Bw /*[G]*/, void* const* y_out /*[G]*/,
                             const int* d_out /*[G]*/, int G, int T, int d_in, int r, float scale, moka_stream_t stream);

/* The launch rule, readable without a device: the number of workgroups moka_dlinear_fwd launches for these widths (each owns a block of
 * 64 output columns of one projection; 128 where 64 would give more than one workgroup per CU of an MI355X, 256 -- and never more than
 * 128: the block's fp32 sums live in registers, wider groups get more workgroups instead; 32 or 16 where the narrower block still gives
 * at most 256, so that a 4096-column projection streams W through every CU).  MOKA_EINVAL for arguments no path accepts. */
int         moka_dlinear_workgroups(const int* d_out /*[G]*/, int G, int d_in, int r);

#ifdef __cplusplus
}
#endif
#endif /* MOKA_DLINEAR_H */
