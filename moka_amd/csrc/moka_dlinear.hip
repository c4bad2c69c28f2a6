// libmoka_dlinear.so: the decode-step adapted projection (include/moka_dlinear.h) -- kernel, launch rule and entry points in one
// translation unit.
//
//     y_g[t] = bf16( x[t] W_g^T + bias_g + scale * (x[t] A_g^T) B_g^T )     g < G <= 3 projections fed by the same x,  t < T <= 16,  bf16
//
// One launch, no workspace; y is written, never read.  The decomposition is moka_decode_kernel's (moka_decode.hip) with W's rows beside
// A's: a workgroup of 8 waves owns a block of CB = 16 NTL output columns of ONE projection, streams those rows of W from HBM exactly
// once and computes the WHOLE h_g = x A_g^T itself (x and A_g are re-read out of L2 / Infinity Cache by every workgroup):
//   phase 1   the waves split d_in in 64-column steps (wave w: steps w, w + 8, ...).  A lane reads 32 contiguous bytes of a row of x,
//             of A_g and of each of the NTL column tiles of W_g per step -- a step is two v_mfma_f32_16x16x32_bf16 per tile whose
//             contraction slots hold columns 16 (l / 16) + 0..7 and + 8..15; all operands use the same map.  The x fragment of a step
//             is loaded once and used against the A tiles and all W tiles.  W goes global -> VGPR (no LDS staging: nothing of it is
//             reused), U steps of loads are requested before the first is consumed.  All loads are unconditional with clamped
//             indices (rows >= T read row T - 1, rank rows >= r read row r - 1, column tiles past d_out the last 16 rows, columns past
//             d_in the last 16): what a clamped load brought is replaced by zeros (columns) or never used (rows).
//   reduce    8 -> 4 -> 2 -> 1 through LDS, the fixed tree of the decode kernel, base sums and h alike: bitwise reproducible, the same
//             for every T, G and column block.  Within a wave the steps are added in step order whatever U is.
//   split     wave 0 scales h in fp32, zeroes rank rows >= r and writes the token-major bf16 [hi(RP) | lo(RP)] rows to LDS, and the
//             fp32 base sums of the NTL column tiles beside them.
//   phase 2   wave ct < NTL takes column tile ct: D[column][token] = base + sum over the 2 RP slots of [B | B][column] . [hi | lo][token]
//             (the base sums are the MFMA's accumulator input), + bias in fp32, ONE rounding to bf16, 8-byte stores for tokens < T.
// A lane of D holds one token and 4 consecutive columns, so rows >= T are simply not stored, and the duplicated rows the clamped loads
// produced never reach memory.
// The block map, the B-fragment load, the reduction tree, the split and the host-side shape checks are moka_step.h's, shared with
// moka_decode.hip.
#include "moka_step.h"
#include "moka_dlinear.h"

namespace {

constexpr int DL_NW = 8;              // waves per workgroup
constexpr int DL_CB_START = 64;       // output columns per workgroup: the decode kernel's 64, doubled while the launch has more than DL_MAX_WG workgroups ...
constexpr int DL_CB_MAX = 128;        // ... up to the block whose fp32 sums, with the loads in flight, fit the registers without a spill,
constexpr int DL_CB_MIN = 16;         // ... and halved (down to one MFMA tile) while the halved launch still has at most DL_MAX_WG
// One workgroup per CU of an MI355X.  The decode kernel's rule stops at 64 columns because every workgroup repeats the pass over x and A_g;
// here a workgroup also streams its rows of W, and a 4096-column projection on 64 of 256 CUs would leave three quarters of the HBM
// channels' requesters idle, so narrow launches are spread further.  Widths that would need a 256-column block for one-per-CU (70B
// gate + up) get more workgroups instead.  A design choice, not a tuned one: other values have not been timed.
constexpr int DL_MAX_WG = 256;

struct DlinearArgs {
    const unsigned short* x;                       // [T][d_in]
    const unsigned short* W[MOKA_MAX_GROUP];       // [C][d_in]
    const unsigned short* bias[MOKA_MAX_GROUP];    // [C] or null
    const unsigned short* A[MOKA_MAX_GROUP];       // [r][d_in]
    const unsigned short* Bw[MOKA_MAX_GROUP];      // [C][r]
    unsigned short* y[MOKA_MAX_GROUP];             // [T][C] out
    int C[MOKA_MAX_GROUP];
    int xend[MOKA_MAX_GROUP];                      // blockIdx.x < xend[g] belongs to projection g (cumulative column blocks)
    int T, d_in, r;
    float scale;
};

// NTL: 16-column tiles of the workgroup's block (CB = 16 NTL), NT: 16-rank tiles (rank pad 16 NT)
template <int NTL, int NT>
__global__ __launch_bounds__(64 * DL_NW) void moka_dlinear_kernel(const DlinearArgs a) {
    constexpr int NW = DL_NW, CB = 16 * NTL;
    constexpr int U = (NTL + NT <= 3) ? 4 : ((NTL + NT <= 8) ? 2 : 1);        // steps of loads in flight per wave (8 (1 + NT + NTL) registers each)
    constexpr int HROW = step_hrow(NT);
    constexpr int FR = NTL + NT;                                              // accumulator fragments of one wave: base tiles, then h tiles
    __shared__ f32x4 s_red[(NW / 2) * FR * 64];
    // after the tree: [0, NTL * 64) the base sums, behind them the [hi | lo] rows (1024 NTL + 32 HROW bytes <= 4096 (NTL + NT))
    unsigned short* const hs = (unsigned short*)(s_red + NTL * 64);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g4 = lane >> 4;
    int g, cblk;
    step_block(a.xend, blockIdx.x, g, cblk);
    const int C = a.C[g], r = a.r, T = a.T, d_in = a.d_in;
    const unsigned short* const Ag = a.A[g];
    const unsigned short* const Bg = a.Bw[g];
    const unsigned short* const Wg = a.W[g];
    const unsigned short* const bg = a.bias[g];
    unsigned short* const yg = a.y[g];
    const int cb0 = cblk * CB;

    // ---- phase 2 operands of the wave's column tile: requested before phase 1, consumed behind it
    // (waves >= NTL and tiles past C request a clamped tile and never use it)
    bf16x8 bfr[NT];
    u32x2 bv = {0u, 0u};
    const int c2 = min(cb0 + 16 * min(wave, NTL - 1), C - 16);
    step_load_b<NT>(Bg + (size_t)(c2 + i) * r, r, g4, bfr);
    if (bg) bv = *(const u32x2*)(bg + c2 + 4 * g4);                           // (wave uniform)

    // ---- phase 1: base^T[column][token] and h^T[rank][token], summed over this wave's 64-column steps
    f32x4 acc[FR];
#pragma unroll
    for (int f = 0; f < FR; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
        const unsigned short* const xrow = a.x + (size_t)min(i, T - 1) * d_in;
        const unsigned short* arow[NT];
        const unsigned short* wrow[NTL];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) arow[nt] = Ag + (size_t)min(16 * nt + i, r - 1) * d_in;
#pragma unroll
        for (int ct = 0; ct < NTL; ++ct) wrow[ct] = Wg + (size_t)(min(cb0 + 16 * ct, C - 16) + i) * d_in;
        const int nst = (d_in + 63) >> 6, nit = (nst + NW - 1) / NW;
        const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int j0 = 0; j0 < nit; j0 += U) {
            bf16x8 xf[U][2], af[U][NT][2], wf[U][NTL][2];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int col = (wave + NW * (j0 + u)) * 64 + 16 * g4;
                ok[u] = col < d_in;                                           // (d_in % 32 == 0: all 16 columns or none)
                const int cc = min(col, d_in - 16);
#pragma unroll
                for (int ct = 0; ct < NTL; ++ct) {
                    wf[u][ct][0] = *(const bf16x8*)(wrow[ct] + cc);
                    wf[u][ct][1] = *(const bf16x8*)(wrow[ct] + cc + 8);
                }
                xf[u][0] = *(const bf16x8*)(xrow + cc);
                xf[u][1] = *(const bf16x8*)(xrow + cc + 8);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    af[u][nt][0] = *(const bf16x8*)(arow[nt] + cc);
                    af[u][nt][1] = *(const bf16x8*)(arow[nt] + cc + 8);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bf16x8 xm = ok[u] ? xf[u][h] : z8;                  // branch-free: the shared operand zeroed past d_in
#pragma unroll
                    for (int ct = 0; ct < NTL; ++ct) acc[ct] = MFMA16(wf[u][ct][h], xm, acc[ct]);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[NTL + nt] = MFMA16(af[u][nt][h], xm, acc[NTL + nt]);
                }
        }
    }

    // ---- the waves' partial sums: 8 -> 4 -> 2 -> 1 in a fixed order
    step_wave_tree<NW>(acc, s_red, wave, lane);

    // ---- wave 0: the base sums as they are; h scaled in fp32 and split into hi + lo, token-major rows [hi(RP) | lo(RP)], rank rows >= r zero
    if (wave == 0) {
#pragma unroll
        for (int ct = 0; ct < NTL; ++ct) s_red[ct * 64 + lane] = acc[ct];
        step_split<NT>(acc, NTL, a.scale, r, hs, i, g4);
    }
    __syncthreads();

    // ---- phase 2: y[token][column] = bf16(base + [B | B][column] . [hi | lo][token] + bias)
    const int c0 = cb0 + 16 * wave;
    if (wave < NTL && c0 < C) {                                               // wave uniform (C % 32 == 0: a tile is whole or absent)
        f32x4 d = s_red[wave * 64 + lane];
#pragma unroll
        for (int j = 0; j < NT; ++j) d = MFMA16(bfr[j], *(const bf16x8*)(hs + (size_t)i * HROW + 32 * j + 8 * g4), d);
        MFMA_SETTLE(d);
        u32x2 res;
        res[0] = f2bf_pk(d[0] + __uint_as_float(bv[0] << 16), d[1] + __uint_as_float(bv[0] & 0xffff0000u));
        res[1] = f2bf_pk(d[2] + __uint_as_float(bv[1] << 16), d[3] + __uint_as_float(bv[1] & 0xffff0000u));
        if (i < T) *(u32x2*)(yg + (size_t)i * C + c0 + 4 * g4) = res;
    }
}

template <int NTL>
void launch_nt(int NT, const DlinearArgs& a, unsigned blocks, hipStream_t st) {
    const dim3 grid(blocks), block(64 * DL_NW);
    if (NT == 1) hipLaunchKernelGGL((moka_dlinear_kernel<NTL, 1>), grid, block, 0, st, a);
    else if (NT == 2) hipLaunchKernelGGL((moka_dlinear_kernel<NTL, 2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((moka_dlinear_kernel<NTL, 4>), grid, block, 0, st, a);
}

// the launch rule: 64 columns per workgroup, doubled while the launch has more than one workgroup per CU and the block fits the
// registers, halved while the halved launch still has at most one workgroup per CU
long launch_rule(const int* d_out, int G, int* CB_out) {
    int CB = DL_CB_START;
    while (count_blocks(d_out, G, CB) > DL_MAX_WG && CB < DL_CB_MAX) CB *= 2;
    while (CB > DL_CB_MIN && count_blocks(d_out, G, CB / 2) <= DL_MAX_WG) CB /= 2;
    *CB_out = CB;
    return count_blocks(d_out, G, CB);
}

}  // namespace

extern "C" {

int moka_dlinear_version(void) { return MOKA_DLINEAR_VERSION; }
const char* moka_dlinear_last_error(void) { return g_err; }
int moka_dlinear_max_tokens(void) { return MOKA_DLINEAR_MAX_TOKENS; }

int moka_dlinear_ok(int T, int d_in, const int* d_out, int G, int r, int dtype) {
    if (dtype != MOKA_BF16 && dtype != MOKA_F32) return fail(MOKA_EINVAL, "moka_dlinear_ok: storage dtype %d is neither MOKA_BF16 nor MOKA_F32", dtype);
    const int rc = check_shape("moka_dlinear_ok", d_in, d_out, G, r);
    if (rc != MOKA_OK) return rc;
    if (dtype != MOKA_BF16) return 0;                                         // fp32 storage: the general path's exact-fp32 kernels
    return (T >= 1 && T <= MOKA_DLINEAR_MAX_TOKENS) ? 1 : 0;
}

int moka_dlinear_workgroups(const int* d_out, int G, int d_in, int r) {
    const int rc = check_shape("moka_dlinear_workgroups", d_in, d_out, G, r);
    if (rc != MOKA_OK) return rc;
    int CB;
    return (int)launch_rule(d_out, G, &CB);
}

int moka_dlinear_fwd(const void* x, const void* const* W, const void* const* bias, const void* const* A, const void* const* Bw,
                     void* const* y_out, const int* d_out, int G, int T, int d_in, int r, float scale, moka_stream_t stream) {
    if (!x || !W || !A || !Bw || !y_out || !d_out) return fail(MOKA_EINVAL, "moka_dlinear_fwd: null pointer");
    const int rc = check_shape("moka_dlinear_fwd", d_in, d_out, G, r);
    if (rc != MOKA_OK) return rc;
    if (T < 1 || T > MOKA_DLINEAR_MAX_TOKENS)
        return fail(MOKA_EINVAL, "moka_dlinear_fwd: T=%d not in 1..%d (moka_dlinear_max_tokens: the base GEMM belongs to the caller)", T, MOKA_DLINEAR_MAX_TOKENS);
    if ((uintptr_t)x & 15) return fail(MOKA_EINVAL, "moka_dlinear_fwd: x must be 16-byte aligned");
    DlinearArgs a;
    memset(&a, 0, sizeof(a));
    a.x = (const unsigned short*)x;
    a.T = T; a.d_in = d_in; a.r = r; a.scale = scale;
    for (int g = 0; g < G; ++g) {
        const void* b = bias ? bias[g] : nullptr;
        const int rcg = check_buffers("moka_dlinear_fwd", "W / bias / A / Bw / y_out", g, {W[g], A[g], Bw[g], y_out[g]}, b);
        if (rcg != MOKA_OK) return rcg;
        a.W[g] = (const unsigned short*)W[g];
        a.bias[g] = (const unsigned short*)b;
        a.A[g] = (const unsigned short*)A[g];
        a.Bw[g] = (const unsigned short*)Bw[g];
        a.y[g] = (unsigned short*)y_out[g];
        a.C[g] = d_out[g];
    }
    int CB;
    const long blocks = launch_rule(d_out, G, &CB);
    fill_xend(a.xend, d_out, G, CB);
    const int NT = rank_pad(r) >> 4;
    const hipStream_t st = (hipStream_t)stream;
    if (CB == 16) launch_nt<1>(NT, a, (unsigned)blocks, st);
    else if (CB == 32) launch_nt<2>(NT, a, (unsigned)blocks, st);
    else if (CB == 64) launch_nt<4>(NT, a, (unsigned)blocks, st);
    else launch_nt<8>(NT, a, (unsigned)blocks, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOKA_ELAUNCH, "moka_dlinear_fwd: %s", hipGetErrorString(e));
    return MOKA_OK;
}

}  // extern "C"
