// Backward kernels of the tiled plan (fp32 training of shapes beyond one workgroup per sample: the CIFAR-shape model).
// Host side: csrc/tiled_train.h.  Every tensor is an HBM-resident NHWC tensor of the forward's workspace ([n][pixel][channel]).
//
//   tb_gemm_kernel<MODE>   one exact-fp32 MFMA contraction (v_mfma_f32_16x16x4f32) with 64 x 64 tiles, K in steps of 16 staged
//                          through LDS; the operands are gathered by mode:
//                            0  strided batched GEMM (attention: dV, dP, dQ, dK; blockIdx.z = sample)
//                            1  data gradient of a conv: dACT[n, v, ci] = sum_{t, co} G[n, o(v, t), co] W[co, ci, t] over the virtual
//                               input grid (3x3 stride 1, the Downsample's stride 2 with its bottom / right pad, 1x1; an upsampled
//                               source gets its 2x2 sum in tb_src_grad_kernel)
//                            2  weight gradient: dW[t][co][ci] = sum_{n, o} G[n, o, co] X[n, v(o, t), ci] over samples x output pixels,
//                               X = the activated input (ACT) or the raw sources (concat A | B, nearest x2 upsampled), split over K
//                               into a slab [split][tap][co][ci] that tb_wgrad_reduce_kernel sums in a fixed order (no atomics)
//   tb_outgrad_kernel      G = s_n * dY in place (+ residual gradient), per-sample column sums (bias, Dense_0)
//   tb_bias_kernel         bias = sum over samples of the column sums; Dense_0 column gradient per sample
//   tb_act_kernel          ACT = dropout(SiLU(GroupNorm(concat(A, B)))) recomputed from the stored input and statistics
//   tb_gn_red_kernel       per (sample, group): sum dxhat, sum dxhat * xhat; per (sample, channel): dgamma, dbeta partials
//   tb_src_grad_kernel     input gradient (GroupNorm backward, or the plain / 2x2-upsample adjoint), added into the sources' twins
//   tb_softmax_bwd_kernel  dS = P o (dP - rowsum(dP o P)) in place
//   tb_resize_bwd_kernel   adjoint of the nearest resize of h onto an odd skip grid, added into the source's twin
#pragma once
#include "common.h"
#include "conv_kernel.h"
#include "tiled_kernels.h"   // ResizeArgs, nearest_src

struct TbGemmArgs {
    int M, N, K;
    // MODE 0
    const float* A; long a_b, a_m, a_k;
    const float* B; long b_b, b_k, b_n;
    float* C; long c_b, c_m, c_n; float alpha;
    // MODE 1 / 2: conv geometry (virtual input Hv x Wv, output Ho x Wo)
    int Hv, Wv, Ho, Wo, stride, pad, ntap, Cin, Cout;
    const float* G;                                   // [n][Ho*Wo][Cout]
    const float* W[3]; int co_blk; long w_co, w_ci, w_t;   // MODE 1: weights in the parameter layout (q | k | v: three matrices of co_blk columns)
    const float* X; const float* X2; int CA, CB, Ha, Wa, up;   // MODE 2: input = concat(X [n][Ha*Wa][CA], X2 [..][CB]), nearest x2 if up
    int kchunk, nsplit;                               // MODE 2: K per split; blockIdx.z = tap * nsplit + split
    float* out;                                       // MODE 1: dACT [n][Hv*Wv][Cin]; MODE 2: slab [nsplit][ntap][Cout][Cin]
};

#define TB_LDS_ROW 68
template <int MODE>
__device__ __forceinline__ float tb_fetch_a(const TbGemmArgs& a, int z, int tap, int m, int k) {
    if (m >= a.M || k >= a.K) return 0.f;
    if (MODE == 0) return a.A[(long)z * a.a_b + (long)m * a.a_m + (long)k * a.a_k];
    if (MODE == 1) {
        const int HWv = a.Hv * a.Wv, n = m / HWv, v = m - n * HWv, vy = v / a.Wv, vx = v - vy * a.Wv;
        const int t = k / a.Cout, co = k - t * a.Cout;
        const int ty = a.ntap == 9 ? t / 3 : 0, tx = a.ntap == 9 ? t % 3 : 0;
        const int ny = vy + a.pad - ty, nx = vx + a.pad - tx;
        if (ny < 0 || nx < 0 || ny % a.stride || nx % a.stride) return 0.f;
        const int oy = ny / a.stride, ox = nx / a.stride;
        if (oy >= a.Ho || ox >= a.Wo) return 0.f;
        return a.G[((long)n * a.Ho * a.Wo + oy * a.Wo + ox) * a.Cout + co];
    }
    (void)tap;
    return a.G[(long)k * a.Cout + m];                 // MODE 2: m = co, k = n * HWo + o
}
template <int MODE>
__device__ __forceinline__ float tb_fetch_b(const TbGemmArgs& a, int z, int tap, int k, int nn) {
    if (nn >= a.N || k >= a.K) return 0.f;
    if (MODE == 0) return a.B[(long)z * a.b_b + (long)k * a.b_k + (long)nn * a.b_n];
    if (MODE == 1) {
        const int t = k / a.Cout, co = k - t * a.Cout, blk = co / a.co_blk;
        return a.W[blk][(long)(co - blk * a.co_blk) * a.w_co + (long)nn * a.w_ci + (long)t * a.w_t];
    }
    const int HWo = a.Ho * a.Wo, n = k / HWo, o = k - n * HWo, oy = o / a.Wo, ox = o - oy * a.Wo;
    const int ty = a.ntap == 9 ? tap / 3 : 0, tx = a.ntap == 9 ? tap % 3 : 0;
    const int vy = oy * a.stride + ty - a.pad, vx = ox * a.stride + tx - a.pad;
    if (vy < 0 || vx < 0 || vy >= a.Hv || vx >= a.Wv) return 0.f;
    const int sy = a.up ? (vy >> 1) : vy, sx = a.up ? (vx >> 1) : vx;
    const long sp = (long)n * a.Ha * a.Wa + sy * a.Wa + sx;
    return nn < a.CA ? a.X[sp * a.CA + nn] : a.X2[sp * a.CB + (nn - a.CA)];
}

template <int MODE>
__global__ __launch_bounds__(RDMI_THREADS) void tb_gemm_kernel(TbGemmArgs a) {
    __shared__ float As[16 * TB_LDS_ROW];             // [k][m]
    __shared__ float Bs[16 * TB_LDS_ROW];             // [k][n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64, z = blockIdx.z;
    int tap = 0, kbeg = 0, kend = a.K;
    if (MODE == 2) {
        tap = z / a.nsplit;
        const int split = z - tap * a.nsplit;
        kbeg = split * a.kchunk; kend = min(a.K, kbeg + a.kchunk);
    }
    // staging order: the operand's contiguous index runs across the work-items
    const bool a_mfast = MODE == 2 || (MODE == 0 && a.a_m == 1);
    const bool b_nfast = MODE == 2 || MODE == 1 || (MODE == 0 && a.b_n == 1);
    float ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid + j * RDMI_THREADS;
            const int mm = a_mfast ? (e & 63) : (e >> 4), ka = a_mfast ? (e >> 6) : (e & 15);
            const int nn = b_nfast ? (e & 63) : (e >> 4), kb = b_nfast ? (e >> 6) : (e & 15);
            ra[j] = k0 + ka < kend ? tb_fetch_a<MODE>(a, z, tap, m0 + mm, k0 + ka) : 0.f;
            rb[j] = k0 + kb < kend ? tb_fetch_b<MODE>(a, z, tap, k0 + kb, n0 + nn) : 0.f;
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, lr = lane & 15, kq = lane >> 4;
    if (kbeg < kend) fetch(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid + j * RDMI_THREADS;
            const int mm = a_mfast ? (e & 63) : (e >> 4), ka = a_mfast ? (e >> 6) : (e & 15);
            const int nn = b_nfast ? (e & 63) : (e >> 4), kb = b_nfast ? (e >> 6) : (e & 15);
            As[ka * TB_LDS_ROW + mm] = ra[j];
            Bs[kb * TB_LDS_ROW + nn] = rb[j];
        }
        __syncthreads();
        if (k0 + 16 < kend) fetch(k0 + 16);           // next step's loads fly under this step's MFMAs
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
            const int kk = k4 * 4 + kq;
            const float a0 = As[kk * TB_LDS_ROW + wm + lr], a1 = As[kk * TB_LDS_ROW + wm + 16 + lr];
            const float b0 = Bs[kk * TB_LDS_ROW + wn + lr], b1 = Bs[kk * TB_LDS_ROW + wn + 16 + lr];
            acc[0][0] = mfma16(a0, b0, acc[0][0]); acc[0][1] = mfma16(a0, b1, acc[0][1]);
            acc[1][0] = mfma16(a1, b0, acc[1][0]); acc[1][1] = mfma16(a1, b1, acc[1][1]);
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + i * 16 + kq * 4 + r, nn = n0 + wn + j * 16 + lr;
                if (m >= a.M || nn >= a.N) continue;
                const float v = acc[i][j][r];
                if (MODE == 0) a.C[(long)z * a.c_b + (long)m * a.c_m + (long)nn * a.c_n] = a.alpha * v;
                else if (MODE == 1) a.out[(long)m * a.Cin + nn] = v;
                else a.out[((long)(z - tap * a.nsplit) * a.ntap + tap) * a.Cout * a.Cin + (long)m * a.Cin + nn] = v;
            }
}

// dW in the parameter layout = sum of the slab's splits (fixed order: run-to-run identical)
__global__ __launch_bounds__(RDMI_THREADS) void tb_wgrad_reduce_kernel(const float* __restrict__ slab, int nsplit, int ntap, int Cout, int Cin,
                                                                       float* W0, float* W1, float* W2, int co_blk, long w_co, long w_ci, long w_t) {
    const long tot = (long)ntap * Cout * Cin;
    const long i = (long)blockIdx.x * RDMI_THREADS + threadIdx.x;
    if (i >= tot) return;
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += slab[(long)k * tot + i];
    const int ci = (int)(i % Cin), co = (int)((i / Cin) % Cout), t = (int)(i / ((long)Cin * Cout));
    const int blk = co / co_blk;
    float* W = blk == 0 ? W0 : blk == 1 ? W1 : W2;
    W[(long)(co - blk * co_blk) * w_co + (long)ci * w_ci + (long)t * w_t] = s;
}

// G[n] = scale / sigma_n * dY[n] (in place when G == dY); dR += G; cs[n][co] = sum over pixels of G
__global__ __launch_bounds__(RDMI_THREADS) void tb_outgrad_kernel(const float* gY, float* G, float* gR, float* __restrict__ cs, int HW, int C, float scale,
                                                                  const float* __restrict__ sig) {
    __shared__ float red[RDMI_THREADS];
    const int n = blockIdx.y, tid = threadIdx.x, col = tid & 63, r = tid >> 6;
    const int co = blockIdx.x * 64 + col;
    const float sc = sig ? scale / sig[n] : scale;
    float s = 0.f;
    if (co < C)
        for (int p = r; p < HW; p += 4) {
            const long i = ((long)n * HW + p) * C + co;
            const float g = gY[i] * sc;
            G[i] = g;
            if (gR) gR[i] += g;
            s += g;
        }
    red[tid] = s;
    __syncthreads();
    if (r == 0 && co < C) cs[(long)n * C + co] = red[tid] + red[tid + 64] + red[tid + 128] + red[tid + 192];
}

// bias gradient (three parameter slices of co_blk columns for q | k | v) and the per-sample Dense_0 column gradient
__global__ __launch_bounds__(RDMI_THREADS) void tb_bias_kernel(const float* __restrict__ cs, int NB, int C, float* b0, float* b1, float* b2, int co_blk,
                                                               float* gdense, int dense_stride, int dense_off) {
    const int co = blockIdx.x * RDMI_THREADS + threadIdx.x;
    if (co >= C) return;
    float s = 0.f;
    for (int n = 0; n < NB; ++n) {
        const float v = cs[(long)n * C + co];
        s += v;
        if (gdense) gdense[(long)n * dense_stride + dense_off + co] = v;
    }
    const int blk = co / co_blk;
    float* b = blk == 0 ? b0 : blk == 1 ? b1 : b2;
    if (b) b[co - blk * co_blk] = s;
}

struct TbGnArgs {
    const float* A; const float* B; int CA, CB, HW, NB;       // sources [n][HW][CA | CB] (no upsampling behind a GroupNorm)
    const float* stats; int G, Cg, act;                        // [n][G][2] (mean, rstd)
    const float* gamma; const float* beta;
    float drop_p; uint32_t op_id; const unsigned long long* seed_dev;
    const float* dACT;                                         // [n][HW][Cin]
    float* ACT;                                                // tb_act_kernel output
    float* red;                                                // [n][G][2]: sum dxhat, sum dxhat * xhat
    float* gslab;                                              // [n][Cin][2]: dgamma, dbeta partials
    float* gA; float* gB;                                      // input-gradient twins (added into; null: no gradient)
    int up, Hv, Wv;                                            // tb_src_grad_kernel without GroupNorm: the virtual grid of dACT
    int has_gn;
};

__device__ __forceinline__ float tb_src(const TbGnArgs& a, long p, int c) { return c < a.CA ? a.A[p * a.CA + c] : a.B[p * a.CB + (c - a.CA)]; }

__global__ __launch_bounds__(RDMI_THREADS) void tb_act_kernel(TbGnArgs a) {
    const int Cin = a.CA + a.CB;
    const long tot = (long)a.NB * a.HW * Cin;
    const long i = (long)blockIdx.x * RDMI_THREADS + threadIdx.x;
    if (i >= tot) return;
    const long p = i / Cin; const int c = (int)(i - p * Cin), n = (int)(p / a.HW), grp = c / a.Cg;
    const float mean = a.stats[((long)n * a.G + grp) * 2], rstd = a.stats[((long)n * a.G + grp) * 2 + 1];
    const float y = (tb_src(a, p, c) - mean) * (rstd * a.gamma[c]) + a.beta[c];
    float v = a.act ? silu_f(y) : y;
    if (a.drop_p > 0.f) v *= dropout_scale(*a.seed_dev, a.op_id, (uint64_t)p * Cin + c, a.drop_p);
    a.ACT[i] = v;
}

// per element of a GroupNorm'd input: xhat and dy = d(pre-activation), recomputed from the stored input, statistics and dACT
__device__ __forceinline__ void tb_gn_elem(const TbGnArgs& a, long p, int c, int n, float& xh, float& dy, float& rstd) {
    const int Cin = a.CA + a.CB, grp = c / a.Cg;
    const float mean = a.stats[((long)n * a.G + grp) * 2];
    rstd = a.stats[((long)n * a.G + grp) * 2 + 1];
    const float x = tb_src(a, p, c);
    xh = (x - mean) * rstd;
    const float y = (x - mean) * (rstd * a.gamma[c]) + a.beta[c];
    float d = a.dACT[p * Cin + c];
    if (a.drop_p > 0.f) d *= dropout_scale(*a.seed_dev, a.op_id, (uint64_t)p * Cin + c, a.drop_p);
    if (a.act) {
        const float s = 1.f / (1.f + __expf(-y));
        d *= s * (1.f + y * (1.f - s));
    }
    dy = d;
}

// one workgroup per (group, sample): the group's Cg channels over all pixels
__global__ __launch_bounds__(RDMI_THREADS) void tb_gn_red_kernel(TbGnArgs a) {
    __shared__ float red[4][RDMI_THREADS];
    const int grp = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int Cin = a.CA + a.CB, pstep = RDMI_THREADS / a.Cg, cl = tid % a.Cg, c = grp * a.Cg + cl;
    float dg = 0.f, db = 0.f, s1 = 0.f, s2 = 0.f;
    if (tid < pstep * a.Cg)
        for (int px = tid / a.Cg; px < a.HW; px += pstep) {
            const long p = (long)n * a.HW + px;
            float xh, dy, rstd;
            tb_gn_elem(a, p, c, n, xh, dy, rstd);
            dg += dy * xh; db += dy;
            const float dxh = dy * a.gamma[c];
            s1 += dxh; s2 += dxh * xh;
        }
    red[0][tid] = dg; red[1][tid] = db; red[2][tid] = s1; red[3][tid] = s2;
    __syncthreads();
    if (tid < a.Cg) {
        float g0 = 0.f, g1 = 0.f;
        for (int j = tid; j < pstep * a.Cg; j += a.Cg) { g0 += red[0][j]; g1 += red[1][j]; }
        a.gslab[((long)n * Cin + c) * 2] = g0; a.gslab[((long)n * Cin + c) * 2 + 1] = g1;
    }
    if (tid == 0) {
        float t1 = 0.f, t2 = 0.f;
        for (int j = 0; j < pstep * a.Cg; ++j) { t1 += red[2][j]; t2 += red[3][j]; }
        a.red[((long)n * a.G + grp) * 2] = t1; a.red[((long)n * a.G + grp) * 2 + 1] = t2;
    }
}

// input gradient over the source grid, added into the sources' gradient twins (every element has one writer per launch)
__global__ __launch_bounds__(RDMI_THREADS) void tb_src_grad_kernel(TbGnArgs a) {
    const int Cin = a.CA + a.CB;
    const int Ha = a.up ? a.Hv / 2 : a.Hv, Wa = a.up ? a.Wv / 2 : a.Wv, HWs = Ha * Wa;
    const long tot = (long)a.NB * HWs * Cin;
    const long i = (long)blockIdx.x * RDMI_THREADS + threadIdx.x;
    if (i >= tot) return;
    const long p = i / Cin; const int c = (int)(i - p * Cin), n = (int)(p / HWs);
    float dx;
    if (a.has_gn) {
        float xh, dy, rstd;
        tb_gn_elem(a, p, c, n, xh, dy, rstd);
        const int grp = c / a.Cg;
        const float inv = 1.f / (float)(a.Cg * a.HW);
        const float t1 = a.red[((long)n * a.G + grp) * 2], t2 = a.red[((long)n * a.G + grp) * 2 + 1];
        dx = rstd * (dy * a.gamma[c] - (t1 + xh * t2) * inv);
    } else if (a.up) {
        const int s = (int)(p - (long)n * HWs), sy = s / Wa, sx = s - sy * Wa;
        const long vb = (long)n * a.Hv * a.Wv;
        dx = 0.f;
        for (int dy2 = 0; dy2 < 2; ++dy2)
            for (int dx2 = 0; dx2 < 2; ++dx2) dx += a.dACT[(vb + (2 * sy + dy2) * a.Wv + 2 * sx + dx2) * Cin + c];
    } else {
        dx = a.dACT[p * Cin + c];
    }
    if (c < a.CA) { if (a.gA) a.gA[p * a.CA + c] += dx; }
    else if (a.gB) a.gB[p * a.CB + (c - a.CA)] += dx;
}

// out[j] = sum_r in[(r * cols + j) * cs + off]  (dgamma / dbeta from the per-sample partials)
__global__ __launch_bounds__(RDMI_THREADS) void tb_rowsum_kernel(const float* __restrict__ in, int rows, int cols, int cs, int off, float* __restrict__ out) {
    const int j = blockIdx.x * RDMI_THREADS + threadIdx.x;
    if (j >= cols) return;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += in[((long)r * cols + j) * cs + off];
    out[j] = s;
}

// Adjoint of nearest_resize_kernel: gS[n][sy][sx][c] += sum of gD over the destination pixels that read (sy, sx).  One work-item per
// SOURCE element: it alone writes that element and adds its destination rows and columns in a fixed order (no atomics: run-to-run
// identical).  With the rule src = floor(dst * in / out) a source row takes the destination rows of one run (one or two of them
// when the grid grows by a row, none when it shrinks past it); rows and columns are found independently.
__global__ __launch_bounds__(RDMI_THREADS) void tb_resize_bwd_kernel(ResizeArgs a, const float* __restrict__ gD, float* gS) {
    const long i = (long)blockIdx.x * RDMI_THREADS + threadIdx.x;
    if (i >= (long)a.NB * a.Hs * a.Ws * a.C) return;
    const int c = (int)(i % a.C);
    const long r = i / a.C;
    const int ps = (int)(r % (a.Hs * a.Ws));
    const long n = r / (a.Hs * a.Ws);
    const int sy = ps / a.Ws, sx = ps - sy * a.Ws;
    float g = 0.f;
    for (int yd = 0; yd < a.Hd; ++yd) {
        if (nearest_src(yd, a.sh, a.Hs) != sy) continue;
        for (int xd = 0; xd < a.Wd; ++xd)
            if (nearest_src(xd, a.sw, a.Ws) == sx) g += gD[((size_t)n * a.Hd * a.Wd + (size_t)yd * a.Wd + xd) * a.C + c];
    }
    gS[i] += g;
}

// dS = P o (dP - sum_j dP o P) over the first L entries of rows of stride ld, one wave per row (in place on dP; a pad [L, ld) is not touched)
__global__ __launch_bounds__(RDMI_THREADS) void tb_softmax_bwd_kernel(const float* __restrict__ P, float* dP, long rows, int L, int ld) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* pr = P + row * ld; float* gr = dP + row * ld;
    float s = 0.f;
    for (int j = lane; j < L; j += 64) s += pr[j] * gr[j];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    for (int j = lane; j < L; j += 64) gr[j] = pr[j] * (gr[j] - s);
}
