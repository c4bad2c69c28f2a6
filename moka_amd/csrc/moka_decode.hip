// libmoka_decode.so: the decode-step adapter kernel (include/moka_decode.h) -- kernel, launch rule and entry points in one translation unit.
//
//     y_g[t] += scale * (x[t] A_g^T) B_g^T        g < G <= 3 projections fed by the same x,  t < T <= 64 tokens,  bf16 storage
//
// One launch, no workspace.  A workgroup of 8 waves owns a block of CB output columns of ONE projection and computes the WHOLE
// h_g = x A_g^T itself (a hand-over between workgroups costs more than the recomputation; x and A_g are re-read out of
// L2 / Infinity Cache by every workgroup):
//   phase 1   the waves split d_in in 64-column steps (wave w: steps w, w + 8, ...).  A lane reads 32 contiguous bytes of a row of x and
//             of A_g per step -- a step is two v_mfma_f32_16x16x32_bf16 whose contraction slots hold columns 16 (l / 16) + 0..7 and
//             + 8..15; both operands use the same map, so the dot products are those of the row-major data.  All loads are unconditional
//             with clamped indices (rows >= T read row T - 1, rank rows >= r read row r - 1, columns past d_in the last 16): what a
//             clamped load brought is replaced by zeros (columns) or never used (rows: see below).
//   reduce    8 -> 4 -> 2 -> 1 through LDS, a fixed tree: bitwise reproducible, and the same for every T (row independence).
//   split     wave 0 scales h in fp32, zeroes rank rows >= r and writes the token-major bf16 [hi(RP) | lo(RP)] rows to LDS.
//   phase 2   a wave takes 16 columns at a time: D[column][token] = sum over the 2 RP slots of [B | B][column] . [hi | lo][token]
//             (RP / 16 MFMAs; rank pad 16: hi and lo share ONE instruction), 8-byte read-modify-write of y for tokens < T.
// A lane of D holds one token and 4 consecutive columns, so rows >= T are simply not stored, and the duplicated rows the clamped loads
// produced never reach memory.
// The block map, the B-fragment load, the reduction tree, the split and the host-side shape checks are moka_step.h's, shared with
// moka_dlinear.hip.
#include "moka_step.h"
#include "moka_decode.h"

namespace {

constexpr int DEC_NW = 8;             // waves per workgroup
constexpr int DEC_CB_MIN = 64;        // output columns per workgroup, doubled until the launch has at most DEC_MAX_WG workgroups
// At most one workgroup per CU of an MI355X: every workgroup repeats phase 1, so a second one on a CU adds a full pass over x and A_g to
// that CU's path to L2.  The cap and the doubling of CB are a design choice, not a tuned one: other values have not been timed.
constexpr int DEC_MAX_WG = 256;

struct DecodeArgs {
    const unsigned short* x;                       // [T][d_in]
    const unsigned short* A[MOKA_MAX_GROUP];       // [r][d_in]
    const unsigned short* Bw[MOKA_MAX_GROUP];      // [C][r]
    unsigned short* y[MOKA_MAX_GROUP];             // [T][C] in/out
    int C[MOKA_MAX_GROUP];
    int xend[MOKA_MAX_GROUP];                      // blockIdx.x < xend[g] belongs to projection g (cumulative column blocks)
    int T, d_in, r, CB;
    float scale;
};

// TT: 16-token tiles (T <= 16 TT), NT: 16-rank tiles (rank pad 16 NT)
template <int TT, int NT>
__global__ __launch_bounds__(64 * DEC_NW) void moka_decode_kernel(const DecodeArgs a) {
    constexpr int NW = DEC_NW;
    constexpr int U = (TT + NT <= 2) ? 8 : ((TT + NT <= 4) ? 4 : 2);         // steps of loads in flight per wave
    constexpr int HROW = step_hrow(NT);
    constexpr int FR = TT * NT;                                               // accumulator fragments of one wave: f = tt * NT + nt
    __shared__ f32x4 s_red[(NW / 2) * FR * 64];                               // (the [hi | lo] rows reuse it: TT (1024 NT + 256) bytes <= 4096 TT NT)
    unsigned short* const hs = (unsigned short*)s_red;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g4 = lane >> 4;
    int g, cblk;
    step_block(a.xend, blockIdx.x, g, cblk);
    const int C = a.C[g], r = a.r, T = a.T, d_in = a.d_in;
    const unsigned short* const Ag = a.A[g];
    const unsigned short* const Bg = a.Bw[g];
    unsigned short* const yg = a.y[g];
    const int ntile = a.CB >> 4;

    // ---- phase 2 operands of the wave's first column tile: requested before phase 1, consumed behind it
    bf16x8 bfr[NT];
    u32x2 yv[TT];
    auto load_tile = [&](int ct) {
        const int c0 = min(cblk * a.CB + 16 * ct, C - 16);                    // (a tile past C is never stored)
        step_load_b<NT>(Bg + (size_t)(c0 + i) * r, r, g4, bfr);
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
            yv[tt] = *(const u32x2*)(yg + (size_t)min(16 * tt + i, T - 1) * C + c0 + 4 * g4);
    };
    // (with fewer column tiles than waves, CB = 64: waves 4..7 request a tile of the next block here, clamped into the buffer, and never
    //  use it -- 1.5 KB of B and y per idle wave, accepted to keep the request unconditional)
    load_tile(wave);

    // ---- phase 1: h^T[rank][token] = sum over this wave's 64-column steps
    f32x4 acc[FR];
#pragma unroll
    for (int f = 0; f < FR; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
        const unsigned short* xrow[TT];
        const unsigned short* arow[NT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) xrow[tt] = a.x + (size_t)min(16 * tt + i, T - 1) * d_in;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) arow[nt] = Ag + (size_t)min(16 * nt + i, r - 1) * d_in;
        const int nst = (d_in + 63) >> 6, nit = (nst + NW - 1) / NW;
        const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int j0 = 0; j0 < nit; j0 += U) {
            bf16x8 xf[U][TT][2], af[U][NT][2];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int col = (wave + NW * (j0 + u)) * 64 + 16 * g4;
                ok[u] = col < d_in;                                           // (d_in % 32 == 0: all 16 columns or none)
                const int cc = min(col, d_in - 16);
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) {
                    xf[u][tt][0] = *(const bf16x8*)(xrow[tt] + cc);
                    xf[u][tt][1] = *(const bf16x8*)(xrow[tt] + cc + 8);
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    af[u][nt][0] = *(const bf16x8*)(arow[nt] + cc);
                    af[u][nt][1] = *(const bf16x8*)(arow[nt] + cc + 8);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt) {
                        const bf16x8 xm = ok[u] ? xf[u][tt][h] : z8;          // branch-free: operands zeroed past d_in
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) acc[tt * NT + nt] = MFMA16(ok[u] ? af[u][nt][h] : z8, xm, acc[tt * NT + nt]);
                    }
        }
    }

    // ---- the waves' partial sums: 8 -> 4 -> 2 -> 1 in a fixed order
    step_wave_tree<NW>(acc, s_red, wave, lane);

    // ---- scale in fp32, split into hi + lo, token-major rows [hi(RP) | lo(RP)]; rank rows >= r are zero
    if (wave == 0) {
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) step_split<NT>(acc, tt * NT, a.scale, r, hs, 16 * tt + i, g4);
    }
    __syncthreads();

    // ---- phase 2: y[token][column] += [B | B][column] . [hi | lo][token]
    bf16x8 hf[TT][NT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
        for (int j = 0; j < NT; ++j) hf[tt][j] = *(const bf16x8*)(hs + (size_t)(16 * tt + i) * HROW + 32 * j + 8 * g4);
    for (int ct = wave; ct < ntile; ct += NW) {
        const int c0 = cblk * a.CB + 16 * ct;
        if (c0 >= C) break;                                                   // wave uniform (C % 32 == 0: a tile is whole or absent)
        if (ct != wave) load_tile(ct);
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NT; ++j) d = MFMA16(bfr[j], hf[tt][j], d);
            MFMA_SETTLE(d);
            const int t = 16 * tt + i;
            const u32x2 o = yv[tt];
            u32x2 res;
            res[0] = f2bf_pk(__uint_as_float(o[0] << 16) + d[0], __uint_as_float(o[0] & 0xffff0000u) + d[1]);
            res[1] = f2bf_pk(__uint_as_float(o[1] << 16) + d[2], __uint_as_float(o[1] & 0xffff0000u) + d[3]);
            if (t < T) *(u32x2*)(yg + (size_t)t * C + c0 + 4 * g4) = res;
        }
    }
}

template <int TT>
void launch_nt(int NT, const DecodeArgs& a, unsigned blocks, hipStream_t st) {
    const dim3 grid(blocks), block(64 * DEC_NW);
    if (NT == 1) hipLaunchKernelGGL((moka_decode_kernel<TT, 1>), grid, block, 0, st, a);
    else if (NT == 2) hipLaunchKernelGGL((moka_decode_kernel<TT, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((moka_decode_kernel<TT, 4>), grid, block, 0, st, a);
}

}  // namespace

extern "C" {

int moka_decode_version(void) { return MOKA_DECODE_VERSION; }
const char* moka_decode_last_error(void) { return g_err; }
int moka_decode_max_tokens(void) { return MOKA_DECODE_MAX_TOKENS; }

int moka_decode_ok(int T, int d_in, const int* d_out, int G, int r, int dtype) {
    if (dtype != MOKA_BF16 && dtype != MOKA_F32) return fail(MOKA_EINVAL, "moka_decode_ok: storage dtype %d is neither MOKA_BF16 nor MOKA_F32", dtype);
    const int rc = check_shape("moka_decode_ok", d_in, d_out, G, r);
    if (rc != MOKA_OK) return rc;
    if (dtype != MOKA_BF16) return 0;                                         // fp32 storage: the general path's exact-fp32 kernels
    return (T >= 1 && T <= MOKA_DECODE_MAX_TOKENS) ? 1 : 0;
}

int moka_decode_fwd(const void* x, const void* const* A, const void* const* Bw, void* const* y_inout, const int* d_out,
                    int G, int T, int d_in, int r, float scale, moka_stream_t stream) {
    if (!x || !A || !Bw || !y_inout || !d_out) return fail(MOKA_EINVAL, "moka_decode_fwd: null pointer");
    const int rc = check_shape("moka_decode_fwd", d_in, d_out, G, r);
    if (rc != MOKA_OK) return rc;
    if (T < 1 || T > MOKA_DECODE_MAX_TOKENS)
        return fail(MOKA_EINVAL, "moka_decode_fwd: T=%d not in 1..%d (moka_decode_max_tokens: use the general path)", T, MOKA_DECODE_MAX_TOKENS);
    if ((uintptr_t)x & 15) return fail(MOKA_EINVAL, "moka_decode_fwd: x must be 16-byte aligned");
    DecodeArgs a;
    memset(&a, 0, sizeof(a));
    a.x = (const unsigned short*)x;
    a.T = T; a.d_in = d_in; a.r = r; a.scale = scale;
    for (int g = 0; g < G; ++g) {
        const int rcg = check_buffers("moka_decode_fwd", "A / Bw / y_inout", g, {A[g], Bw[g], y_inout[g]});
        if (rcg != MOKA_OK) return rcg;
        a.A[g] = (const unsigned short*)A[g];
        a.Bw[g] = (const unsigned short*)Bw[g];
        a.y[g] = (unsigned short*)y_inout[g];
        a.C[g] = d_out[g];
    }
    // launch rule: 64 columns per workgroup, doubled until the launch has at most one workgroup per CU
    int CB = DEC_CB_MIN;
    while (count_blocks(d_out, G, CB) > DEC_MAX_WG) CB *= 2;
    const long blocks = count_blocks(d_out, G, CB);
    a.CB = CB;
    fill_xend(a.xend, d_out, G, CB);
    const int TT = (T + 15) >> 4, NT = rank_pad(r) >> 4;
    const hipStream_t st = (hipStream_t)stream;
    if (TT == 1) launch_nt<1>(NT, a, (unsigned)blocks, st);
    else if (TT == 2) launch_nt<2>(NT, a, (unsigned)blocks, st);
    else if (TT == 3) launch_nt<3>(NT, a, (unsigned)blocks, st);
    else launch_nt<4>(NT, a, (unsigned)blocks, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOKA_ELAUNCH, "moka_decode_fwd: %s", hipGetErrorString(e));
    return MOKA_OK;
}

}  // extern "C"
