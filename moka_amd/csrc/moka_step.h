// The core the two decode-step kernels share (moka_decode.hip: the adapter term onto a base output; moka_dlinear.hip: base GEMV and adapter
// term in one launch).  Included by those two translation units and by nothing else; no part of libmoka_hip.so.
//
// Both kernels promise bitwise reproducibility with row, grouping and column-block independence.  That promise rests on the reduction
// tree and the hi + lo split below, so there is one copy of each.  What differs per kernel -- the argument struct, the phase-1 load /
// MFMA loop, the epilogue and the launch rule -- stays in its .hip.
#pragma once
#include "moka_device.h"

#include <initializer_list>

// ---------------------------------------------------------------------------------------------------------------- device
// blockIdx.x -> (projection g, column block cblk of g): block b < xend[g] belongs to projection g (cumulative column blocks)
static __device__ __forceinline__ void step_block(const int (&xend)[MOKA_MAX_GROUP], int bid, int& g, int& cblk) {
    g = (bid >= xend[0] ? 1 : 0) + (bid >= xend[1] ? 1 : 0);
    cblk = bid - (g == 0 ? 0 : xend[g - 1]);
}

// The phase-2 B operand of one 16-column tile: NT fragments of this lane's row of B_g [C][r] (brow = B_g + column * r).  Rows of B that
// are whole 16-byte vectors (r % 8 == 0) are read as such, others element by element; indices are clamped into the row, rank slots >= r
// are zero.  (r by reference, as the decode kernel's tile lambda sees it: by value the compiler lifts the clamped index out of that
// kernel's tile loop and holds it across phase 1 -- two more VGPRs at rank pad 32.)
template <int NT>
static __device__ __forceinline__ void step_load_b(const unsigned short* brow, const int& r, int g4, bf16x8 (&bfr)[NT]) {
    constexpr int RP = 16 * NT;
    const bool vecB = (r & 7) == 0;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int k0 = (32 * j + 8 * g4) & (RP - 1);                          // rank of this lane's contraction slots (rank pad 16: hi | lo in one step)
        bf16x8 v;
        if (vecB) {
            v = *(const bf16x8*)(brow + min(k0, r - 8));
            if (k0 >= r) v = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned short w = brow[min(k0 + e, r - 1)];
                v[e] = (k0 + e < r) ? (short)w : (short)0;
            }
        }
        bfr[j] = v;
    }
}

// The NW waves' partial sums, FR accumulator fragments each: 8 -> 4 -> 2 -> 1 through s_red[(NW / 2) * FR * 64] in a fixed order; the
// total is wave 0's acc.  Ends behind a barrier: s_red is free for reuse.
template <int NW, int FR>
static __device__ __forceinline__ void step_wave_tree(f32x4 (&acc)[FR], f32x4* s_red, int wave, int lane) {
#pragma unroll
    for (int f = 0; f < FR; ++f) MFMA_SETTLE(acc[f]);
#pragma unroll
    for (int half = NW / 2; half >= 1; half >>= 1) {
        if (wave >= half && wave < 2 * half) {
#pragma unroll
            for (int f = 0; f < FR; ++f) s_red[((wave - half) * FR + f) * 64 + lane] = acc[f];
        }
        __syncthreads();
        if (wave < half) {
#pragma unroll
            for (int f = 0; f < FR; ++f) acc[f] += s_red[(wave * FR + f) * 64 + lane];
        }
        __syncthreads();
    }
}

constexpr int step_hrow(int NT) { return 2 * 16 * NT + 8; }                   // bf16 per [hi | lo] row in LDS (16 bytes of padding)

// The NT rank tiles acc[f0 .. f0 + NT) of one 16-token tile (an MFMA result: lane (i, g4) holds token i, ranks 4 g4 + 0..3 of each tile):
// scaled in fp32, rank rows >= r zeroed, split into hi + lo and written to the token-major row hs[trow][hi(RP) | lo(RP)].
template <int NT, int FR>
static __device__ __forceinline__ void step_split(const f32x4 (&acc)[FR], int f0, float scale, int r, unsigned short* hs, int trow, int g4) {
    constexpr int RP = 16 * NT, HROW = step_hrow(NT);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        unsigned short hi[4], lo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = 16 * nt + 4 * g4 + e;
            const float v = (k < r) ? scale * acc[f0 + nt][e] : 0.f;
            split_hi_lo(v, hi[e], lo[e]);
        }
        unsigned short* row = hs + (size_t)trow * HROW + 16 * nt + 4 * g4;
        *(u32x2*)row = (u32x2){(unsigned)hi[0] | ((unsigned)hi[1] << 16), (unsigned)hi[2] | ((unsigned)hi[3] << 16)};
        *(u32x2*)(row + RP) = (u32x2){(unsigned)lo[0] | ((unsigned)lo[1] << 16), (unsigned)lo[2] | ((unsigned)lo[3] << 16)};
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
// (anonymous namespace: each shared object has its own error buffer)
namespace {

thread_local char g_err[384] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int rank_pad(int r) { return (r < 1 || r > 64) ? MOKA_EINVAL : (r <= 16 ? 16 : (r <= 32 ? 32 : 64)); }

// what no path accepts (the messages of include/moka_hip.h's entry points); T is judged by the callers
int check_shape(const char* fn, int d_in, const int* d_out, int G, int r) {
    if (G < 1 || G > MOKA_MAX_GROUP) return fail(MOKA_EINVAL, "%s: G=%d not in 1..%d", fn, G, MOKA_MAX_GROUP);
    if (!d_out) return fail(MOKA_EINVAL, "%s: null pointer (d_out)", fn);
    if (rank_pad(r) < 0) return fail(MOKA_EINVAL, "%s: rank %d not in 1..64", fn, r);
    if (d_in < 32 || (d_in % 32) != 0) return fail(MOKA_EINVAL, "%s: feature width %d must be a positive multiple of 32", fn, d_in);
    for (int g = 0; g < G; ++g)
        if (d_out[g] < 32 || (d_out[g] % 32) != 0) return fail(MOKA_EINVAL, "%s: feature width %d must be a positive multiple of 32", fn, d_out[g]);
    return MOKA_OK;
}

// the buffers of projection g: every one of `must` is there, and those and `may` (null: absent) are 16-byte aligned
int check_buffers(const char* fn, const char* names, int g, std::initializer_list<const void*> must, const void* may = nullptr) {
    uintptr_t bits = (uintptr_t)may;
    for (const void* p : must) {
        if (!p) return fail(MOKA_EINVAL, "%s: null pointer (projection %d)", fn, g);
        bits |= (uintptr_t)p;
    }
    if (bits & 15) return fail(MOKA_EINVAL, "%s: %s of projection %d must be 16-byte aligned", fn, names, g);
    return MOKA_OK;
}

// workgroups of a launch with CB output columns per workgroup
long count_blocks(const int* d_out, int G, int CB) {
    long blocks = 0;
    for (int g = 0; g < G; ++g) blocks += (d_out[g] + CB - 1) / CB;
    return blocks;
}

void fill_xend(int (&xend)[MOKA_MAX_GROUP], const int* d_out, int G, int CB) {
    int end = 0;
    for (int g = 0; g < MOKA_MAX_GROUP; ++g) {
        if (g < G) end += (d_out[g] + CB - 1) / CB;
        xend[g] = end;                                                        // (absent projections: no block reaches them)
    }
}

}  // namespace
