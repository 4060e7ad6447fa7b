// LayerNorm forward / backward over the fp32 residual stream (K3 prologue of SURVEY.md 2.2).
// Replaces nn.LayerNorm at decoder_Uformer.py:567,594,666,744 / encoder_Uformer.py:549,577,641,680
// and the LN in front of the encoder heads (encoder_Uformer.py:941).  HBM-bound: one pass, 16-byte
// loads, G lanes per row (G = 16/32/64 by width) so narrow rows (C = 28, 56) do not idle a wave.
//   fwd : y[T] = (x - mean) * rstd * gamma + beta ; saves mean, rstd (fp32)
//   bwd : dx[f32] = (dres?) + rstd * (g - mean(g) - xhat * mean(g*xhat)),  g = dy * gamma
//         dgamma += sum_rows dy * xhat ; dbeta += sum_rows dy      (block partials by plain stores -> fw_slab_reduce)
//         dy: T rows, or the unfolded f32 slab of the split-K input-gradient GEMM in front (fw_layernorm_bwd_slab)
//   learnable window modulator of the decoder blocks (decoder_Uformer.py:536-539,687-691):
//   fwd : y[T] = LN(x) * gamma + beta + mod[window position of the row]      (a compile-time branch of the forward kernel)
//   bwd : dmod[p] += sum of dy over the rows at window position p            (slices by plain stores -> fw_slab_reduce, no atomics)
#include "fw_common.h"
#include <stdlib.h>

namespace {

constexpr int NVMAX = 4;   // float4 per lane: C <= 4*4*64 = 1024

template <int G> FW_DEV float group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T> struct RawV;                         // 4 elements of T kept packed until they are consumed
template <> struct RawV<float> {
    f32x4 v;
    FW_MEM void load(const float* p) { v = *reinterpret_cast<const f32x4*>(p); }
    FW_MEM void unpack(float* f) const { f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3]; }
};
template <> struct RawV<bf16raw> {
    uint2 v;
    FW_MEM void load(const bf16raw* p) { v = *reinterpret_cast<const uint2*>(p); }
    FW_MEM void unpack(float* f) const {
        f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
        f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    }
};

// Both kernels are pure streams (read a row, two group reductions, write a row), i.e. bound by how many bytes a CU keeps in
// flight: with ONE row per lane group outstanding (the first form of these kernels) a CU had ~40 KB requested at a time and the
// pass ran at 2.8 TB/s.  Now a lane group owns U rows per step -- all their loads are issued back to back from CLAMPED coordinates
// (no branch between them), then the rows are reduced and written -- and the per-lane arrays are sized by NV = ceil(C / 4 / G),
// not by the C = 1024 maximum.  G lanes per row (16 / 32 / 64 by width) so that narrow rows (C = 28, 56) do not idle a wave.
//
// MOD (fw_layernorm_mod_fwd): the decoder's learnable window modulator (decoder_Uformer.py:536-539,687-691) rides on the same stream.
// The reference adds an [64][C] table to the 64 tokens of every 8x8 window AFTER norm1, the cyclic shift and the window partition; the
// token of row r = (b, yy, xx) of the [B*H*W, C] stream sits at window position p(r) = ((yy - s) & 7) * 8 + ((xx - s) & 7)
// (roll(-s) puts pixel yy at rolled row (yy - s) mod H, and 8 | H), so  y[r] = T(LN(x[r]) * gamma + beta + mod[p(r)]).  The table rows
// (<= 229 KB in all, L2-resident) are requested with the U rows of x, from the same clamped coordinates.  MOD is a compile-time branch:
// the plain instantiations (MOD = false) compile every modulator statement out and never read the four trailing arguments.
template <typename T, int G, int NV, int U, bool MOD = false>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, T* __restrict__ y, long ldy,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int rows,
                                                     int C, float eps, const float* __restrict__ mod, int H, int W, int shift) {
    constexpr int RPB = 256 / G;
    const int gl = threadIdx.x % G, gr = threadIdx.x / G;
    const int nv = C >> 2;
    const long r0 = (long)blockIdx.x * RPB * U;
    f32x4 v[U][NV];
    f32x4 mv[MOD ? U : 1][MOD ? NV : 1];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const long row = r0 + u * RPB + gr;
        const long rc = row < rows ? row : rows - 1;
        const float* xr = x + rc * ldx;
        const float* mr = nullptr;
        if (MOD) {
            const unsigned iy = (unsigned)rc / (unsigned)W;           // rows is an int: 32-bit divisions
            const int xx = (int)((unsigned)rc - iy * (unsigned)W), yy = (int)(iy % (unsigned)H);
            mr = mod + (long)((((yy - shift) & 7) << 3) + ((xx - shift) & 7)) * C;
        }
#pragma unroll
        for (int t = 0; t < NV; ++t) {
            const int c4 = gl + G * t;
            v[u][t] = *reinterpret_cast<const f32x4*>(xr + (c4 < nv ? c4 : nv - 1) * 4);
            if (MOD) mv[u][t] = *reinterpret_cast<const f32x4*>(mr + (c4 < nv ? c4 : nv - 1) * 4);
        }
    }
    f32x4 gam[NV], bet[NV];
#pragma unroll
    for (int t = 0; t < NV; ++t) {
        const int c4 = gl + G * t < nv ? gl + G * t : nv - 1;
        gam[t] = *reinterpret_cast<const f32x4*>(gamma + c4 * 4);
        bet[t] = *reinterpret_cast<const f32x4*>(beta + c4 * 4);
    }
    const float invc = 1.0f / C;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const long row = r0 + u * RPB + gr;
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < NV; ++t) {
            if (gl + G * t >= nv) v[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            s += v[u][t][0] + v[u][t][1] + v[u][t][2] + v[u][t][3];
        }
        const float mu = group_sum<G>(s) * invc;
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < NV; ++t) {
            if (gl + G * t < nv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = v[u][t][e] - mu; q += d * d; }
            }
        }
        const float rs = rsqrtf(group_sum<G>(q) * invc + eps);
        if (row >= rows) continue;
        if (gl == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
        for (int t = 0; t < NV; ++t) {
            const int c4 = gl + G * t;
            if (c4 < nv) {
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (v[u][t][e] - mu) * rs * gam[t][e] + bet[t][e];
                if (MOD) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] += mv[u][t][e];
                }
                T* yp = y + row * ldy + c4 * 4;
                if (sizeof(T) == 4) *reinterpret_cast<f32x4*>(yp) = f32x4{o[0], o[1], o[2], o[3]};
                else *reinterpret_cast<uint2*>(yp) = make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
            }
        }
    }
}

// dy of one lane vector summed from the nz slices of a split-K slab (p: the vector in slice 0, zs: floats between slices), in the
// association of slab_reduce_kernel (fw_elem.hip) with the whole z range in one block: partial sum j takes slices j, j + 4, ..., each
// started from zero and advanced by the same unrolled pairing, and the total is s0 + ((s1 + s2) + s3) -- the same bits as the fold.
// nz <= 4 (the deep stages split 2 or 3 ways) is one independent load per slice under wave-uniform branches.
FW_DEV f32x4 slab_dy_sum(const float* __restrict__ p, int nz, long zs) {
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (nz <= 4) {
        s[0] += *reinterpret_cast<const f32x4*>(p);
        if (nz > 1) s[1] += *reinterpret_cast<const f32x4*>(p + zs);
        if (nz > 2) s[2] += *reinterpret_cast<const f32x4*>(p + 2 * zs);
        if (nz > 3) s[3] += *reinterpret_cast<const f32x4*>(p + 3 * zs);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int z = j;
            for (; z + 12 < nz; z += 16) {
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(p + (long)z * zs);
                const f32x4 a1 = *reinterpret_cast<const f32x4*>(p + (long)(z + 4) * zs);
                const f32x4 a2 = *reinterpret_cast<const f32x4*>(p + (long)(z + 8) * zs);
                const f32x4 a3 = *reinterpret_cast<const f32x4*>(p + (long)(z + 12) * zs);
                s[j] += (a0 + a1) + (a2 + a3);
            }
            for (; z < nz; z += 4) s[j] += *reinterpret_cast<const f32x4*>(p + (long)z * zs);
        }
    }
    return s[0] + ((s[1] + s[2]) + s[3]);
}
template <typename T> FW_DEV void raw_from_sum(RawV<T>& r, const f32x4& s);
template <> FW_SPEC void raw_from_sum<float>(RawV<float>& r, const f32x4& s) { r.v = s; }                     // parity mode: no rounding
template <> FW_SPEC void raw_from_sum<bf16raw>(RawV<bf16raw>& r, const f32x4& s) {                            // as cast_rows_kernel rounds
    r.v = make_uint2(pack_bf2(s[0], s[1]), pack_bf2(s[2], s[3]));
}

// Each block walks row groups blockIdx.x, blockIdx.x + gridDim.x, ... of RPB * U rows; column partial sums stay in registers.
// SLAB: dy is not a T matrix but the unfolded f32 slab of the split-K input-gradient GEMM in front (nz slices of rows x C contiguous
// partials, zstride floats apart): the lane sums its vector from the slices and rounds it to T exactly as fw_slab_reduce ->
// fw_cast_rows would have, so dx, twin and the column partials are the bits of that three-launch chain without its two passes.
template <typename T, int G, int NV, int U, int TPB, bool SLAB>
__global__ __launch_bounds__(TPB) void ln_bwd_kernel(const T* __restrict__ dy, long lddy, const float* __restrict__ slab, int nz, long zstride,
                                                     const float* __restrict__ x, long ldx,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ dres, long lddres,
                                                     float* __restrict__ dx, long lddx, float* __restrict__ partial,
                                                     long pstride, int rows, int C, T* __restrict__ twin, long ldtw,
                                                     const float* __restrict__ twscale, int tw_rows_per_scale) {
    constexpr int RPB = TPB / G;
    const int gl = threadIdx.x % G, gr = threadIdx.x / G;
    const int nv = C >> 2;
    const float invc = 1.0f / C;
    f32x4 gam[NV], dg[NV], db[NV];
    bool cok[NV];
#pragma unroll
    for (int t = 0; t < NV; ++t) {
        const int c4 = gl + G * t;
        cok[t] = c4 < nv;
        gam[t] = cok[t] ? *reinterpret_cast<const f32x4*>(gamma + c4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        dg[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        db[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (long r0 = (long)blockIdx.x * RPB * U; r0 < rows; r0 += (long)gridDim.x * RPB * U) {
        // ---- every load of the U rows first ----
        f32x4 xv[U][NV], rr[U][NV];
        RawV<T> dr[U][NV];
        float mu[U], rs[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = r0 + u * RPB + gr;
            const long rc = row < rows ? row : rows - 1;
            mu[u] = mean[rc]; rs[u] = rstd[rc];
#pragma unroll
            for (int t = 0; t < NV; ++t) {
                const int cc = (cok[t] ? gl + G * t : nv - 1) * 4;
                xv[u][t] = *reinterpret_cast<const f32x4*>(x + rc * ldx + cc);
                if (!SLAB) dr[u][t].load(dy + rc * lddy + cc);
                if (dres) rr[u][t] = *reinterpret_cast<const f32x4*>(dres + rc * lddres + cc);
            }
        }
        if (SLAB) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long row = r0 + u * RPB + gr;
                const long rc = row < rows ? row : rows - 1;
#pragma unroll
                for (int t = 0; t < NV; ++t) {
                    const int cc = (cok[t] ? gl + G * t : nv - 1) * 4;
                    raw_from_sum<T>(dr[u][t], slab_dy_sum(slab + rc * C + cc, nz, zstride));
                }
            }
        }
        // ---- then row by row ----
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long row = r0 + u * RPB + gr;
            const bool live = row < rows;
            f32x4 xh[NV], g[NV];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int t = 0; t < NV; ++t) {
                float d[4];
                dr[u][t].unpack(d);
                const bool ok = live && cok[t];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float de = ok ? d[e] : 0.f;
                    xh[t][e] = ok ? (xv[u][t][e] - mu[u]) * rs[u] : 0.f;
                    g[t][e] = de * gam[t][e];
                    dg[t][e] += de * xh[t][e];
                    db[t][e] += de;
                    s1 += g[t][e];
                    s2 += g[t][e] * xh[t][e];
                }
            }
            s1 = group_sum<G>(s1) * invc;
            s2 = group_sum<G>(s2) * invc;
            if (!live) continue;
            const float sc = (twin && twscale) ? twscale[row / tw_rows_per_scale] : 1.0f;
#pragma unroll
            for (int t = 0; t < NV; ++t) {
                if (!cok[t]) continue;
                const int c4 = gl + G * t;
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = rs[u] * (g[t][e] - s1 - xh[t][e] * s2);
                if (dres) o += rr[u][t];
                *reinterpret_cast<f32x4*>(dx + row * lddx + c4 * 4) = o;
                if (twin) {                                  // the operand copy the preceding Linear's backward needs: T(dx * DropPath scale)
                    T* tp = twin + row * ldtw + c4 * 4;
                    if (sizeof(T) == 4) *reinterpret_cast<f32x4*>(tp) = o * sc;
                    else *reinterpret_cast<uint2*>(tp) = make_uint2(pack_bf2(o[0] * sc, o[1] * sc), pack_bf2(o[2] * sc, o[3] * sc));
                }
            }
        }
    }
    // block reduction of the column partials over the RPB row groups in a FIXED order: every row group stores its registers to its own
    // LDS row (16-byte stores, no zero-fill, no atomics), then each column is summed over the row groups 0, 1, ... by one thread --
    // the same (rows, C) gives the same dgamma / dbeta bits on every call.
    constexpr int COLS = NV * 4 * G;
    __shared__ float red[RPB][2][COLS];
#pragma unroll
    for (int t = 0; t < NV; ++t) {
        const int c4 = gl + G * t;
        *reinterpret_cast<f32x4*>(&red[gr][0][c4 * 4]) = dg[t];
        *reinterpret_cast<f32x4*>(&red[gr][1][c4 * 4]) = db[t];
    }
    __syncthreads();
    // block partials [block][dgamma(Cp) | dbeta(Cp)]: plain stores; fw_slab_reduce folds them (thousands of blocks adding
    // atomically into the same C words serialise in L2 and cost more than the whole LayerNorm pass)
    float* pp = partial + (long)blockIdx.x * pstride;
    const int Cp = (int)(pstride >> 1);
    for (int c = threadIdx.x; c < Cp; c += TPB) {
        float a = 0.f, b = 0.f;
        if (c < C) {
            a = red[0][0][c]; b = red[0][1][c];
#pragma unroll
            for (int k = 1; k < RPB; ++k) { a += red[k][0][c]; b += red[k][1][c]; }
        }
        pp[c] = a;
        pp[Cp + c] = b;
    }
}

// rows per lane group and step (U) by the number of 16-byte vectors a lane holds per row (NV): about 4 row-vectors in flight
template <typename T, int G, int NV, int U>
int ln_fwd_launch(const float* x, long ldx, const float* g, const float* b, void* y, long ldy, float* mean,
                  float* rstd, int rows, int C, float eps, hipStream_t st) {
    const int rpb = 256 / G * U;
    hipLaunchKernelGGL((ln_fwd_kernel<T, G, NV, U>), dim3(fw_cdiv(rows, rpb)), dim3(256), 0, st, x, ldx, g, b, (T*)y, ldy,
                       mean, rstd, rows, C, eps, (const float*)nullptr, 1, 1, 0);
    FW_LAUNCH_RET();
}
template <typename T, int G, int NV, int U>
int ln_mod_fwd_launch(const float* x, long ldx, const float* g, const float* b, const float* mod, void* y, long ldy, float* mean,
                      float* rstd, int rows, int C, int H, int W, int shift, float eps, hipStream_t st) {
    const int rpb = 256 / G * U;
    hipLaunchKernelGGL((ln_fwd_kernel<T, G, NV, U, true>), dim3(fw_cdiv(rows, rpb)), dim3(256), 0, st, x, ldx, g, b, (T*)y, ldy,
                       mean, rstd, rows, C, eps, mod, H, W, shift);
    FW_LAUNCH_RET();
}
static inline int ln_group(int C) { return C <= 32 ? 8 : (C <= 64 ? 16 : (C <= 128 ? 32 : 64)); }
static inline int ln_rows_per_step(int C) { return C <= 256 ? 4 : (C <= 512 ? 2 : 1); }
// Blocks of the backward pass (the one source of the number of `partial` rows).  Every block ends in a fold of its column partials and
// writes 2 C floats for fw_slab_reduce to re-read.  While that fold was a zero-fill of 2048 LDS words plus 2 C LDS float atomics per
// row group it cost ~9 us a block -- more than the rows of a deep-stage launch -- and the caps below 1024 existed to buy it back with
// few blocks that walk many rows (averages then at caps 1024 / 512 / 256, C = 896: 36.2 / 26.7 / 22.1 us, C = 448: 25.6 / 23.4 /
// 22.3 us, C = 224: 25.7 / 24.4 / 27.9 us, C <= 112: 46.5 / 47.4 / 57.8 us).  With the ordered store-then-sum fold the same grids
// run (rows x C, us on cold operands, bf16 dy, before -> after at 256 threads): 1024 x 896 16.7 -> 7.5, 4096 x 896 27.1 -> 17.8,
// 4096 x 448 15.5 -> 10.6, 16384 x 448 34.9 -> 30.2, 16384 x 224 21.7 -> 18.9.  What is left for the cap to decide is small;
// measured again per workgroup size (threads / cap):
//   4096 x 896  : 256/256 17.8, 256/512 17.2, 512/256 16.6, 512/512 18.6, 1024/256 17.1     (1024 x 896: 7.4 at 256 and 512, 10.2 at 1024)
//   16384 x 448 : 256/256 30.2, 256/512 27.7, 512/256 27.4, 512/512 25.7, 1024/256 26.5     (4096 x 448: 10.6 / 10.0 / 9.8 / 9.9 / 10.4)
//   65536 x 224 : 256/512 48.7, 256/1024 47.1, 512/256 49.1, 512/512 47.3, 512/1024 48.0    (16384 x 224: 17.1 / 16.2 / 17.1 / 16.2 / 16.3)
// 512 threads (8 waves a CU behind one partial row; 1024 threads leave the slab form 128 registers and it spills) with cap 256 above
// C = 512 and 512 above C = 128.  The C <= 128 forms keep 256 threads and cap 1024.
constexpr int LN_BWD_WIDE_TPB = 512;     // threads of a backward workgroup at C > 128 (G = 64: 8 row groups); 256 below
static inline int ln_bwd_grid(int rows, int C) {
    const int tpb = C > 128 ? LN_BWD_WIDE_TPB : 256;
    const int cap = C > 512 ? 256 : (C > 128 ? 512 : 1024);
    return min(fw_cdiv(rows, tpb / ln_group(C) * ln_rows_per_step(C)), cap);
}

// dy / lddy: T [rows][lddy], or -- slab != null -- the unfolded split-K slab (slab, nz, zstride) of rows x C contiguous partials
struct LnBwdArgs {
    const void* dy; long lddy; const float* slab; int nz; long zstride;
    const float* x; long ldx; const float* g; const float* mean; const float* rstd; const float* dres; long lddres;
    float* dx; long lddx; float* partial; long pstride; int rows, C; void* twin; long ldtw; const float* twscale; int twrps;
};
template <typename T, int G, int NV, int U, int TPB>
int ln_bwd_launch(const LnBwdArgs& a, hipStream_t st) {
    const dim3 grid(ln_bwd_grid(a.rows, a.C)), block(TPB);
#define LN_BK(SLAB)                                                                                                                  \
    hipLaunchKernelGGL((ln_bwd_kernel<T, G, NV, U, TPB, SLAB>), grid, block, 0, st, (const T*)a.dy, a.lddy, a.slab, a.nz, a.zstride, a.x, \
                       a.ldx, a.g, a.mean, a.rstd, a.dres, a.lddres, a.dx, a.lddx, a.partial, a.pstride, a.rows, a.C, (T*)a.twin, a.ldtw, \
                       a.twscale, a.twrps)
    if (a.slab) LN_BK(true);
    else LN_BK(false);
#undef LN_BK
    FW_LAUNCH_RET();
}
template <typename T>
int ln_bwd_dispatch(const LnBwdArgs& a, hipStream_t st) {
    const int C = a.C;                             // (G, NV, U) as LN_DISPATCH; the workgroup size as ln_bwd_grid counts it
    return C <= 32    ? ln_bwd_launch<T, 8, 1, 4, 256>(a, st)
           : C <= 64  ? ln_bwd_launch<T, 16, 1, 4, 256>(a, st)
           : C <= 128 ? ln_bwd_launch<T, 32, 1, 4, 256>(a, st)
           : C <= 256 ? ln_bwd_launch<T, 64, 1, 4, LN_BWD_WIDE_TPB>(a, st)
           : C <= 512 ? ln_bwd_launch<T, 64, 2, 2, LN_BWD_WIDE_TPB>(a, st)
                      : ln_bwd_launch<T, 64, 4, 1, LN_BWD_WIDE_TPB>(a, st);
}

// ---- gradient of the window modulator: dmod[p][c] = sum over the rows r with p(r) = p of dy[r][c] -----------------------------------
// Every window holds each p once, so a sum has n = rows / 64 terms; the rows that share p are 8 tokens apart along x and 8 image rows
// apart along y.  A workgroup owns one yq = (yy - s) & 7, a column chunk and one of nz slices of the n terms: its 8 groups of 32 lanes
// take the eight xq = (xx - s) & 7, so the 8 * TG tokens the block requests at a time are consecutive in memory.  Inside a group CL
// lanes span the chunk's columns (E elements each: 16 bytes of f32, 16 or -- rows not 16-byte aligned -- 8 bytes of bf16) and the
// TG = 32 / CL token groups take every TG-th term; LD loads are issued from clamped terms before any is added.  The token groups are
// folded through LDS in a fixed order and slice z stores its [64][C] partial with plain stores: no atomics, the same bits every call.
template <typename T, int E> struct ModV;
template <> struct ModV<float, 4> {
    f32x4 v;
    FW_MEM void load(const float* p) { v = *reinterpret_cast<const f32x4*>(p); }
    FW_MEM void add(float* a) const { a[0] += v[0]; a[1] += v[1]; a[2] += v[2]; a[3] += v[3]; }
};
template <> struct ModV<bf16raw, 4> {
    RawV<bf16raw> r;
    FW_MEM void load(const bf16raw* p) { r.load(p); }
    FW_MEM void add(float* a) const { float f[4]; r.unpack(f); a[0] += f[0]; a[1] += f[1]; a[2] += f[2]; a[3] += f[3]; }
};
template <> struct ModV<bf16raw, 8> {
    uint4 v;
    FW_MEM void load(const bf16raw* p) { v = *reinterpret_cast<const uint4*>(p); }
    FW_MEM void add(float* a) const {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { a[2 * i] += __uint_as_float(w[i] << 16); a[2 * i + 1] += __uint_as_float(w[i] & 0xffff0000u); }
    }
};

constexpr int MOD_LD = 8;        // loads a lane has in flight

template <typename T, int E, int CL>
__global__ __launch_bounds__(256) void mod_bwd_kernel(const T* __restrict__ dy, long lddy, float* __restrict__ partial, int n, int per,
                                                      int C, int W, int shift) {
    constexpr int TG = 32 / CL;
    const int cl = threadIdx.x % CL, tg = threadIdx.x / CL % TG, xq = threadIdx.x / 32;
    const int yq = blockIdx.y, z = blockIdx.z;
    const int col = (blockIdx.x * CL + cl) * E;
    const bool cok = col < C;                                  // E | C: a vector is inside the row or outside it
    const int W8 = W >> 3;
    const int g0 = (yq + shift) & 7, x0 = (xq + shift) & 7;      // first image row (of all B * H) and first token of this (yq, xq)
    const int lo = z * per, hi = min(n, lo + per);              // terms of this slice: term u = (image row g0 + 8 (u / W8), token x0 + 8 (u % W8))
    const T* base = dy + (cok ? col : 0);
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    for (int u = lo + tg; u < hi; u += TG * MOD_LD) {
        ModV<T, E> v[MOD_LD];
#pragma unroll
        for (int i = 0; i < MOD_LD; ++i) {
            const int uc = min(u + i * TG, hi - 1);
            const int j = uc / W8, k = uc - j * W8;
            v[i].load(base + ((long)(g0 + 8 * j) * W + x0 + 8 * k) * lddy);
        }
#pragma unroll
        for (int i = 0; i < MOD_LD; ++i) {
            if (u + i * TG < hi) v[i].add(acc);
        }
    }
    if (TG > 1) {
        __shared__ float red[256 * E];
#pragma unroll
        for (int e = 0; e < E; ++e) red[threadIdx.x * E + e] = acc[e];
        __syncthreads();
        if (tg == 0) {
#pragma unroll
            for (int t = 1; t < TG; ++t) {
#pragma unroll
                for (int e = 0; e < E; ++e) acc[e] += red[(threadIdx.x + t * CL) * E + e];
            }
        }
    }
    if (tg != 0 || !cok) return;
    float* pp = partial + ((long)z * 64 + yq * 8 + xq) * C + col;
#pragma unroll
    for (int e = 0; e < E; e += 4) *reinterpret_cast<f32x4*>(pp + e) = f32x4{acc[e], acc[e + 1], acc[e + 2], acc[e + 3]};
}

// Slices of the n = rows / 64 terms.  Each slice writes a [64][C] f32 partial that the fold re-reads -- 2 nz / n of the bf16 bytes of
// dy, twice -- so a slice keeps at least 16 terms (12.5 %); 32 slices put 8 * 32 * chunks = 256 .. 1024 workgroups on the 256 CUs at
// the decoder's four shapes (batch 16, 128 x 128: n = 4096 / 1024 / 256 / 64 -> nz = 32 / 32 / 16 / 4), and the fold of <= 32 slices
// needs no split of its own.
static inline int mod_bwd_slices(int rows, int C) {
    const int n = rows / 64;
    return max(1, min(32, n / 16));
}

template <typename T, int E>
int mod_bwd_launch(const void* dy, long lddy, float* partial, int rows, int C, int W, int shift, hipStream_t st) {
    const int n = rows / 64, nz = mod_bwd_slices(rows, C), per = fw_cdiv(n, nz), nvr = C / E;
#define MOD_B(CL)                                                                                                              \
    hipLaunchKernelGGL((mod_bwd_kernel<T, E, CL>), dim3(fw_cdiv(nvr, CL), 8, nz), dim3(256), 0, st, (const T*)dy, lddy, partial, n, \
                       per, C, W, shift)
    if (nvr <= 8) MOD_B(8);
    else if (nvr <= 16) MOD_B(16);
    else MOD_B(32);
#undef MOD_B
    FW_LAUNCH_RET();
}

// (G, NV, U) by row width
#define LN_DISPATCH(FN, T, ...)                                    \
    (C <= 32 ? FN<T, 8, 1, 4>(__VA_ARGS__)                         \
     : C <= 64 ? FN<T, 16, 1, 4>(__VA_ARGS__)                      \
     : C <= 128 ? FN<T, 32, 1, 4>(__VA_ARGS__)                     \
     : C <= 256 ? FN<T, 64, 1, 4>(__VA_ARGS__)                     \
     : C <= 512 ? FN<T, 64, 2, 2>(__VA_ARGS__)                     \
                : FN<T, 64, 4, 1>(__VA_ARGS__))

}  // namespace

extern "C" int fw_layernorm_fwd(int dtype, const float* x, long ldx, const float* gamma, const float* beta, void* y,
                                long ldy, float* mean, float* rstd, int rows, int C, float eps, void* stream) {
    FW_CHECK_ARG(rows > 0 && C > 0 && C % 4 == 0 && C <= 1024 && ldx % 4 == 0 && ldy % 4 == 0);
    FW_CHECK_ARG(x && gamma && beta && y && mean && rstd);
    hipStream_t st = (hipStream_t)stream;
#define LN_F(T) LN_DISPATCH(ln_fwd_launch, T, x, ldx, gamma, beta, y, ldy, mean, rstd, rows, C, eps, st)
    return dtype == FW_DT_BF16 ? LN_F(bf16raw) : LN_F(float);
#undef LN_F
}

// Number of block partials fw_layernorm_bwd writes for (rows, C): the caller provides `partial` f32 [blocks][2 * roundup(C, 4)].
extern "C" int fw_layernorm_bwd_blocks(int rows, int C) { return ln_bwd_grid(rows, C); }

// dx = (dres?) + LN'(dy).  The per-block column sums of dy*xhat / dy go to `partial` (plain stores, row = [dgamma | dbeta]) and
// are folded into dgamma / dbeta (accumulated) by fw_slab_reduce, launched here on the same stream -- unless both are null.
extern "C" int fw_slab_reduce(const float* slab, int nz, long n, long zstride, float* dst, int accumulate, float* dst2, long off2, long n2,
                              void* stream);
// dy_slab != null: dy is the unfolded slab of the split-K input-gradient GEMM in front -- nz slices, zstride floats apart, each rows x C
// contiguous f32 partials -- and the kernel sums and rounds it as fw_slab_reduce -> fw_cast_rows would have (dy / lddy are not read).
extern "C" int fw_layernorm_bwd_slab(int dtype, const void* dy, long lddy, const float* dy_slab, int nz, long zstride, const float* x, long ldx,
                                     const float* gamma, const float* mean, const float* rstd, const float* dres, long lddres, float* dx,
                                     long lddx, float* dgamma, float* dbeta, float* partial, int rows, int C, void* twin, long ldtw,
                                     const float* twscale, int tw_rows_per_scale, void* stream) {
    FW_CHECK_ARG(rows > 0 && C > 0 && C % 4 == 0 && C <= 1024 && ldx % 4 == 0 && lddx % 4 == 0);
    FW_CHECK_ARG(x && gamma && mean && rstd && dx && partial && ((dgamma && dbeta) || (!dgamma && !dbeta)));
    FW_CHECK_ARG(!twin || (ldtw % 4 == 0 && (!twscale || tw_rows_per_scale > 0)));
    if (dy_slab) FW_CHECK_ARG(nz > 0 && zstride % 4 == 0 && zstride >= (long)rows * C && ((uintptr_t)dy_slab & 15) == 0);
    else FW_CHECK_ARG(dy && lddy % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    const long pstride = 2L * C;
    const LnBwdArgs a{dy, lddy, dy_slab, nz, zstride, x, ldx, gamma, mean, rstd, dres, lddres, dx, lddx, partial, pstride, rows, C,
                      twin, ldtw, twscale, tw_rows_per_scale};
    const int rc = dtype == FW_DT_BF16 ? ln_bwd_dispatch<bf16raw>(a, st) : ln_bwd_dispatch<float>(a, st);
    if (rc || !dgamma) return rc;                  // dgamma == dbeta == null: the caller folds the partials later (fw_slab_reduce_multi)
    return fw_slab_reduce(partial, ln_bwd_grid(rows, C), C, pstride, dgamma, 1, dbeta, C, C, stream);
}

extern "C" int fw_layernorm_bwd2(int dtype, const void* dy, long lddy, const float* x, long ldx, const float* gamma,
                                 const float* mean, const float* rstd, const float* dres, long lddres, float* dx,
                                 long lddx, float* dgamma, float* dbeta, float* partial, int rows, int C, void* twin, long ldtw,
                                 const float* twscale, int tw_rows_per_scale, void* stream) {
    FW_CHECK_ARG(dy);
    return fw_layernorm_bwd_slab(dtype, dy, lddy, nullptr, 0, 0, x, ldx, gamma, mean, rstd, dres, lddres, dx, lddx, dgamma, dbeta, partial,
                                 rows, C, twin, ldtw, twscale, tw_rows_per_scale, stream);
}

extern "C" int fw_layernorm_bwd(int dtype, const void* dy, long lddy, const float* x, long ldx, const float* gamma,
                                const float* mean, const float* rstd, const float* dres, long lddres, float* dx,
                                long lddx, float* dgamma, float* dbeta, float* partial, int rows, int C, void* stream) {
    return fw_layernorm_bwd2(dtype, dy, lddy, x, ldx, gamma, mean, rstd, dres, lddres, dx, lddx, dgamma, dbeta, partial, rows, C,
                             nullptr, 0, nullptr, 1, stream);
}

// y[r] = T(LN(x[r]) * gamma + beta + mod[p(r)]),  p(r) = ((yy - shift) & 7) * 8 + ((xx - shift) & 7) for row r = (b, yy, xx) of the
// [B*H*W, C] stream; mod: f32 [64][C], 16-byte aligned.  mean / rstd as fw_layernorm_fwd writes them.
extern "C" int fw_layernorm_mod_fwd(int dtype, const float* x, long ldx, const float* gamma, const float* beta, const float* mod, void* y,
                                    long ldy, float* mean, float* rstd, int rows, int C, int H, int W, int shift, float eps, void* stream) {
    FW_CHECK_ARG(rows > 0 && C > 0 && C % 4 == 0 && C <= 1024 && ldx % 4 == 0 && ldy % 4 == 0);
    FW_CHECK_ARG(x && gamma && beta && mod && y && mean && rstd && ((uintptr_t)mod & 15) == 0);
    FW_CHECK_ARG(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && rows % ((long)H * W) == 0 && shift >= 0 && shift < 8);
    hipStream_t st = (hipStream_t)stream;
#define LN_F(T) LN_DISPATCH(ln_mod_fwd_launch, T, x, ldx, gamma, beta, mod, y, ldy, mean, rstd, rows, C, H, W, shift, eps, st)
    return dtype == FW_DT_BF16 ? LN_F(bf16raw) : LN_F(float);
#undef LN_F
}

// Number of slices fw_modulator_bwd writes for (rows, C): the caller provides `partial` f32 [slices][64][C], 16-byte aligned.
extern "C" int fw_modulator_bwd_blocks(int rows, int C) { return mod_bwd_slices(rows, C); }

// dmod[p][c] += sum over the rows r with p(r) = p of dy[r][c]  (dmod: f32 [64][C], ACCUMULATED).  dy is read once; slice z of the
// rows / 64 terms stores partial[z] and fw_slab_reduce folds the slices into dmod on the same stream, every address by one
// read-modify-write -- unless dmod is null: the caller folds `partial` later (fw_slab_reduce / fw_slab_reduce_multi).
extern "C" int fw_modulator_bwd(int dtype, const void* dy, long lddy, float* dmod, float* partial, int rows, int C, int H, int W, int shift,
                                void* stream) {
    FW_CHECK_ARG(rows > 0 && C > 0 && C % 4 == 0 && C <= 1024 && lddy % 4 == 0 && lddy >= C);
    FW_CHECK_ARG(dy && partial && ((uintptr_t)partial & 15) == 0);
    FW_CHECK_ARG(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && rows % ((long)H * W) == 0 && shift >= 0 && shift < 8);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (dtype != FW_DT_BF16) {
        FW_CHECK_ARG(((uintptr_t)dy & 15) == 0);
        rc = mod_bwd_launch<float, 4>(dy, lddy, partial, rows, C, W, shift, st);
    } else if (C % 8 == 0 && lddy % 8 == 0 && ((uintptr_t)dy & 15) == 0) {
        rc = mod_bwd_launch<bf16raw, 8>(dy, lddy, partial, rows, C, W, shift, st);
    } else {
        FW_CHECK_ARG(((uintptr_t)dy & 7) == 0);
        rc = mod_bwd_launch<bf16raw, 4>(dy, lddy, partial, rows, C, W, shift, st);
    }
    if (rc || !dmod) return rc;
    return fw_slab_reduce(partial, mod_bwd_slices(rows, C), 64L * C, 64L * C, dmod, 2, nullptr, 0, 0, stream);
}
