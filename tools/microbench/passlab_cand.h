// Candidate kernels for tools/microbench/passlab.hip (design probes, not product code).
#pragma once
#include <functional>
#define NFAM 8

// ---- cand0: the x stream of moka_xa_kernel<1,NG> alone (same block shape, same loads, two groups in flight, no weights,
//      no MFMA, no LDS, no stores): what the access pattern itself costs behind a read-modify-write launch
template <int NG>
__global__ void __launch_bounds__(512) cand_read_frag(const unsigned char* x, int T, int C, unsigned* out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    TRACE_DECL(4);
    TRACE(0);
    const int grp0 = blockIdx.y * NG;
    const int c0 = blockIdx.x * 512 + 64 * wave;
    unsigned acc = 0;
    auto issue = [&](bf16x8 (&F)[2][2], int grp_) {
        const int grp = min(grp_, grp0 + NG - 1);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const size_t rowoff = (size_t)min((grp << 5) + 16 * st + i, T - 1) * C;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) F[st][kk] = *(const bf16x8*)(x + (rowoff + c0 + 32 * kk + 8 * g) * 2);
        }
    };
    auto eat = [&](bf16x8 (&F)[2][2]) {
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) { union { bf16x8 b; unsigned u[4]; } v; v.b = F[st][kk]; acc ^= v.u[0] ^ v.u[1] ^ v.u[2] ^ v.u[3]; }
    };
    bf16x8 FA[2][2], FB[2][2];
    issue(FA, grp0);
#pragma unroll 1
    for (int gi = 0; gi < NG; gi += 2) {
        issue(FB, grp0 + gi + 1);
        eat(FA);
        if (gi == 0) TRACE(1);
        issue(FA, grp0 + gi + 2);
        eat(FB);
        if (gi == 0) TRACE(2);
    }
    if (acc == 0x12345678u) out[0] = acc;
    TRACE(7);
}

// ---- cand1: row-linear stream: block = 256 threads walking a contiguous token run of whole rows, U x 4 KB in flight
template <int U>
__global__ void __launch_bounds__(256) cand_read_rows(const unsigned char* x, size_t bytes_per_block, unsigned* out) {
    TRACE_DECL(5);
    TRACE(0);
    const uint4* p = (const uint4*)(x + (size_t)blockIdx.x * bytes_per_block) + threadIdx.x;
    const size_t n = bytes_per_block / 16;
    unsigned acc = 0;
    for (size_t k = 0; k + (U - 1) * 256 < n; k += U * 256) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = p[k + u * 256];
#pragma unroll
        for (int u = 0; u < U; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
        if (k == 0) TRACE(1);
    }
    if (acc == 0x12345678u) out[0] = acc;
    TRACE(7);
}


// ---- cand2: cand0 plus, one at a time, what moka_xa2_kernel has besides its loads (VAR bit 1: routing byte loads, 2: a 200-byte
//      by-value argument struct, 4: 33 KB of dynamic LDS touched once, 8: the LDS staging of the block's routing bytes)
struct BigArgs { const unsigned char* x; const unsigned char* pad[12]; const unsigned char* tok_mod; float s[4]; int T, C, r, M; unsigned d[15]; };
template <int NG, int VAR>
__global__ void __launch_bounds__(512) cand_read_frag2(const BigArgs a, unsigned* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem2[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    TRACE_DECL(6);
    TRACE(0);
    const int grp0 = blockIdx.y * NG;
    const int c0 = blockIdx.x * 512 + 64 * wave;
    unsigned acc = 0;
    if (VAR & 8) { if (tid < NG * 32) smem2[tid] = a.tok_mod[grp0 * 32 + tid]; }
    auto issue = [&](bf16x8 (&F)[2][2], int (&mr)[2], int grp_) {
        const int grp = min(grp_, grp0 + NG - 1);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            if (VAR & 1) mr[st] = a.tok_mod[(grp << 5) + 16 * st + i]; else mr[st] = 0;
            const size_t rowoff = (size_t)min((grp << 5) + 16 * st + i, a.T - 1) * a.C;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) F[st][kk] = *(const bf16x8*)(a.x + (rowoff + c0 + 32 * kk + 8 * g) * 2);
        }
    };
    auto eat = [&](bf16x8 (&F)[2][2], int (&mr)[2]) {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            acc += mr[st];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) { union { bf16x8 b; unsigned u[4]; } v; v.b = F[st][kk]; acc ^= v.u[0] ^ v.u[1] ^ v.u[2] ^ v.u[3]; }
        }
        if (VAR & 4) { *(unsigned*)(smem2 + 1024 + 4 * tid) = acc; }
    };
    bf16x8 FA[2][2], FB[2][2]; int mA[2], mB[2];
    issue(FA, mA, grp0);
#pragma unroll 1
    for (int gi = 0; gi < NG; gi += 2) {
        issue(FB, mB, grp0 + gi + 1);
        eat(FA, mA);
        if (gi == 0) TRACE(1);
        issue(FA, mA, grp0 + gi + 2);
        eat(FB, mB);
        if (gi == 0) TRACE(2);
    }
    if (VAR & 2) acc += a.d[3] + a.d[14] + (unsigned)(size_t)a.pad[11] + (unsigned)a.s[3];
    if (VAR & 8) { __syncthreads(); acc += smem2[(tid * 7) & 127]; }
    if (acc == 0x12345678u) out[0] = acc;
    TRACE(7);
}

static void cand_main(unsigned short* const* x, unsigned short* const* y, unsigned short* const* A, const uint8_t* tok_mod, float* part, int T,
                      std::function<void(int)> front, std::function<void(const char*)> report, std::function<void()> clear) {
    unsigned* out; (void)hipMalloc(&out, 64);
    auto go = [&](const char* title, std::function<void(int)> k) {
        for (int it = 0; it < 4; ++it) { front(it % 4); k(it % 4); }
        (void)hipDeviceSynchronize();
        hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0);
        for (int it = 0; it < 12; ++it) { front(it % 4); k(it % 4); }
        (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1);
        clear(); front(1); k(1); front(2); k(2); clear(); front(3); k(3);
        char t2[256]; snprintf(t2, sizeof(t2), "%s   (sequence avg %.1f us)", title, ms * 1e3 / 12);
        report(t2);
    };
    const int C = 4096;
    go("front + cand0 read_frag<4> C=4096 (512 blocks)", [&](int s) { hipLaunchKernelGGL((cand_read_frag<4>), dim3(C / 512, T / 128), dim3(512), 0, 0, (const unsigned char*)x[s], T, C, out); });
    {
        BigArgs ba; memset(&ba, 0, sizeof(ba));
        ba.T = T; ba.C = C; ba.tok_mod = tok_mod;
        go("front + cand2 var 0", [&](int s) { ba.x = (const unsigned char*)x[s]; hipLaunchKernelGGL((cand_read_frag2<4, 0>), dim3(C / 512, T / 128), dim3(512), 0, 0, ba, out); });
        go("front + cand2 var 1 (routing byte loads)", [&](int s) { ba.x = (const unsigned char*)x[s]; hipLaunchKernelGGL((cand_read_frag2<4, 1>), dim3(C / 512, T / 128), dim3(512), 0, 0, ba, out); });
        go("front + cand2 var 2 (args struct read)", [&](int s) { ba.x = (const unsigned char*)x[s]; hipLaunchKernelGGL((cand_read_frag2<4, 2>), dim3(C / 512, T / 128), dim3(512), 0, 0, ba, out); });
        go("front + cand2 var 4 (33 KB LDS)", [&](int s) { ba.x = (const unsigned char*)x[s]; hipLaunchKernelGGL((cand_read_frag2<4, 4>), dim3(C / 512, T / 128), dim3(512), 33 * 1024, 0, ba, out); });
        go("front + cand2 var 8 (routing bytes staged in LDS)", [&](int s) { ba.x = (const unsigned char*)x[s]; hipLaunchKernelGGL((cand_read_frag2<4, 8>), dim3(C / 512, T / 128), dim3(512), 33 * 1024, 0, ba, out); });
        go("front + cand2 var 15 (all)", [&](int s) { ba.x = (const unsigned char*)x[s]; hipLaunchKernelGGL((cand_read_frag2<4, 15>), dim3(C / 512, T / 128), dim3(512), 33 * 1024, 0, ba, out); });
    }
    go("front + cand0 read_frag<8> C=4096 (256 blocks)", [&](int s) { hipLaunchKernelGGL((cand_read_frag<8>), dim3(C / 512, T / 256), dim3(512), 0, 0, (const unsigned char*)x[s], T, C, out); });
    go("front + cand1 read_rows<4> 67 MB, 256 blocks", [&](int s) { hipLaunchKernelGGL((cand_read_rows<4>), dim3(256), dim3(256), 0, 0, (const unsigned char*)x[s], (size_t)T * C * 2 / 256, out); });
    go("front + cand1 read_rows<4> 67 MB, 1024 blocks", [&](int s) { hipLaunchKernelGGL((cand_read_rows<4>), dim3(1024), dim3(256), 0, 0, (const unsigned char*)x[s], (size_t)T * C * 2 / 1024, out); });
    go("front + cand1 read_rows<8> 67 MB, 512 blocks", [&](int s) { hipLaunchKernelGGL((cand_read_rows<8>), dim3(512), dim3(256), 0, 0, (const unsigned char*)x[s], (size_t)T * C * 2 / 512, out); });
}
