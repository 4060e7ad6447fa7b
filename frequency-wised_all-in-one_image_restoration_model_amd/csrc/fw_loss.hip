// Structural-similarity loss term of the training step (fwair.h: fw_ssim11_loss; utils/pytorch_ssim/__init__.py:19-43).
//
// S(a, b) with the 11x11 Gaussian window (sigma 1.5, zero padding 5), its mean over every pixel, and the gradient of that mean
// with respect to a -- value and gradient in ONE launch, no intermediate map in HBM:
//   mu_a, mu_b, E_aa, E_bb, E_ab = conv(a), conv(b), conv(a a), conv(b b), conv(a b)
//   s_aa = E_aa - mu_a^2, s_bb = E_bb - mu_b^2, s_ab = E_ab - mu_a mu_b
//   A1 = 2 mu_a mu_b + C1, A2 = 2 s_ab + C2, B1 = mu_a^2 + mu_b^2 + C1, B2 = s_aa + s_bb + C2, S = A1 A2 / (B1 B2)
//   d mean(S) / d a[q] = (conv(G_mu)[q] + 2 a[q] conv(G_aa)[q] + b[q] conv(G_ab)[q]) / N
//   G_aa = -S / B2,  G_ab = 2 A1 / (B1 B2),  G_mu = 2 mu_b (A2 - A1) / (B1 B2) - 2 mu_a S / B1 + 2 mu_a S / B2
// (the window is symmetric, hence its own adjoint; zero padding of the adjoint: G counts as zero outside the image).
#include "fw_common.h"

// No contraction in this file: products and sums round where they are written (fmaf where one rounding is meant).  The sums of the
// a == b case then cancel exactly (A1 == B1, A2 == B2 bit for bit), and `da + v` of the accumulating form adds the very v that the
// plain form stores.
#pragma clang fp contract(off)

namespace {

constexpr int SS_T = 32;                 // a workgroup's tile of output pixels (SS_T x SS_T of one plane)
constexpr int SS_HALO = SS_T + 20;       // inputs: the tile and 10 pixels around it (two convolutions of radius 5)
constexpr int SS_RING = SS_T + 10;       // the five maps and the three G maps: the tile and 5 pixels around it
constexpr int SS_TPB = 256;
constexpr int SS_RING_PER_THREAD = (SS_RING * SS_RING + SS_TPB - 1) / SS_TPB;
constexpr float SS_C1 = 0.01f * 0.01f, SS_C2 = 0.03f * 0.03f;

// exp(-(x - 5)^2 / (2 * 1.5^2)), x = 0..10, rounded to f32 and divided by their f32 sum (pytorch_ssim gaussian(11, 1.5)): the f32 values
FW_DEV float ss_tap(int k) {
    constexpr float g[11] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                             0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
    return g[k];
}

// grid: planes * tiles_y * tiles_x workgroups of 256 threads; workgroup -> (plane, tile).  LDS 65 328 bytes: two workgroups per CU.
//   1. a, b on the 52 x 52 halo, zeros outside the image
//   2. row pass of the five maps, 52 rows x 42 columns               (lanes along x: consecutive LDS words, no bank conflict)
//   3. column pass on the 42 x 42 ring, S and the three G maps in registers (zero outside the image); S summed over the tile's own
//      pixels; then the G maps replace the row-pass results in LDS
//   4. row pass of the three G maps, 42 rows x 32 columns
//   5. column pass for the 32 x 32 tile, a thread owning 4 consecutive pixels of a row (16-byte LDS reads, a 16-byte store)
// Every da element is written by exactly one thread, no atomics: the gradient is bit-reproducible.  The VALUE takes one float
// atomicAdd per workgroup (as l1_loss_kernel does), so its last bits depend on the order in which the workgroups arrive.
__global__ __launch_bounds__(SS_TPB) void ssim11_loss_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ da,
                                                             int H, int W, int tiles_x, int tiles_y, float gs, float fN, int accumulate,
                                                             int vec, float* __restrict__ loss) {
    __shared__ float sa[SS_HALO * SS_HALO], sb[SS_HALO * SS_HALO];
    __shared__ __attribute__((aligned(16))) float tmp[5 * SS_HALO * SS_RING];
    __shared__ float red[SS_TPB / 64];
    const int t = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int y0 = (tile / tiles_x) * SS_T, x0 = (tile % tiles_x) * SS_T;
    const long pbase = (long)plane * H * W;

    for (int idx = t; idx < SS_HALO * SS_HALO; idx += SS_TPB) {
        const int i = idx / SS_HALO, j = idx - i * SS_HALO;
        const int y = y0 - 10 + i, x = x0 - 10 + j;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const long o = pbase + (long)y * W + x;
        sa[idx] = in ? a[o] : 0.f;
        sb[idx] = in ? b[o] : 0.f;
    }
    __syncthreads();

    constexpr int MAP5 = SS_HALO * SS_RING;
    for (int idx = t; idx < MAP5; idx += SS_TPB) {
        const int i = idx / SS_RING, c = idx - i * SS_RING;
        const float* pa = sa + i * SS_HALO + c;
        const float* pb = sb + i * SS_HALO + c;
        float ma = 0.f, mb = 0.f, eaa = 0.f, ebb = 0.f, eab = 0.f;
#pragma unroll
        for (int l = 0; l < 11; ++l) {
            const float va = pa[l], vb = pb[l], g = ss_tap(l);
            ma = fmaf(g, va, ma);
            mb = fmaf(g, vb, mb);
            eaa = fmaf(g, va * va, eaa);
            ebb = fmaf(g, vb * vb, ebb);
            eab = fmaf(g, va * vb, eab);
        }
        tmp[idx] = ma; tmp[MAP5 + idx] = mb; tmp[2 * MAP5 + idx] = eaa; tmp[3 * MAP5 + idx] = ebb; tmp[4 * MAP5 + idx] = eab;
    }
    __syncthreads();

    float gmu[SS_RING_PER_THREAD], gaa[SS_RING_PER_THREAD], gab[SS_RING_PER_THREAD];
    float ssum = 0.f;
#pragma unroll
    for (int it = 0; it < SS_RING_PER_THREAD; ++it) {
        const int idx = t + it * SS_TPB;
        gmu[it] = gaa[it] = gab[it] = 0.f;
        if (idx >= SS_RING * SS_RING) continue;
        const int r = idx / SS_RING, c = idx - r * SS_RING;
        const int y = y0 - 5 + r, x = x0 - 5 + c;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;
        const float* p = tmp + r * SS_RING + c;
        float ma = 0.f, mb = 0.f, eaa = 0.f, ebb = 0.f, eab = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float g = ss_tap(k);
            ma = fmaf(g, p[k * SS_RING], ma);
            mb = fmaf(g, p[MAP5 + k * SS_RING], mb);
            eaa = fmaf(g, p[2 * MAP5 + k * SS_RING], eaa);
            ebb = fmaf(g, p[3 * MAP5 + k * SS_RING], ebb);
            eab = fmaf(g, p[4 * MAP5 + k * SS_RING], eab);
        }
        const float ma2 = ma * ma, mb2 = mb * mb, mab = ma * mb;
        const float saa = eaa - ma2, sbb = ebb - mb2, sab = eab - mab;
        const float A1 = 2.f * mab + SS_C1, A2 = 2.f * sab + SS_C2;
        const float B1 = (ma2 + mb2) + SS_C1, B2 = (saa + sbb) + SS_C2;
        const float den = B1 * B2;
        const float S = (A1 * A2) / den;
        gaa[it] = -S / B2;
        gab[it] = (2.f * A1) / den;
        gmu[it] = ((2.f * mb) * (A2 - A1)) / den - ((2.f * ma) * S) / B1 + ((2.f * ma) * S) / B2;
        if (r >= 5 && r < 5 + SS_T && c >= 5 && c < 5 + SS_T) ssum += S;
    }
    __syncthreads();                                           // every column pass has read the row-pass maps
    constexpr int MAPG = SS_RING * SS_RING;
#pragma unroll
    for (int it = 0; it < SS_RING_PER_THREAD; ++it) {
        const int idx = t + it * SS_TPB;
        if (idx < MAPG) { tmp[idx] = gmu[it]; tmp[MAPG + idx] = gaa[it]; tmp[2 * MAPG + idx] = gab[it]; }
    }
    __syncthreads();

    constexpr int MAPH = SS_RING * SS_T;
    float* h2 = tmp + 3 * MAPG;                                // 16-byte aligned: 3 * 42 * 42 * 4 bytes = 1323 * 16
    static_assert((3 * MAPG) % 4 == 0 && 3 * MAPG + 3 * MAPH <= 5 * MAP5, "G maps and their row pass share the row-pass buffer");
    for (int idx = t; idx < MAPH; idx += SS_TPB) {
        const int r = idx / SS_T, x = idx - r * SS_T;
        const float* p = tmp + r * SS_RING + x;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int l = 0; l < 11; ++l) {
            const float g = ss_tap(l);
            s0 = fmaf(g, p[l], s0);
            s1 = fmaf(g, p[MAPG + l], s1);
            s2 = fmaf(g, p[2 * MAPG + l], s2);
        }
        h2[idx] = s0; h2[MAPH + idx] = s1; h2[2 * MAPH + idx] = s2;
    }
    __syncthreads();

    if (da) {
        const int y = t >> 3, x4 = (t & 7) << 2;
        const int gy = y0 + y, gx = x0 + x4;
        if (gy < H && gx < W) {
            f32x4 cm = {0.f, 0.f, 0.f, 0.f}, caa = cm, cab = cm;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float g = ss_tap(k);
                const float* p = h2 + (y + k) * SS_T + x4;
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(p);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(p + MAPH);
                const f32x4 v2 = *reinterpret_cast<const f32x4*>(p + 2 * MAPH);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    cm[j] = fmaf(g, v0[j], cm[j]);
                    caa[j] = fmaf(g, v1[j], caa[j]);
                    cab[j] = fmaf(g, v2[j], cab[j]);
                }
            }
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float av = sa[(y + 10) * SS_HALO + x4 + 10 + j], bv = sb[(y + 10) * SS_HALO + x4 + 10 + j];
                v[j] = gs * ((cm[j] + (2.f * av) * caa[j]) + bv * cab[j]);
            }
            float* q = da + pbase + (long)gy * W + gx;
            if (vec) {                                         // W % 4 == 0 and da 16-byte aligned: gx + 3 < W, the row segment is aligned
                if (accumulate) v = *reinterpret_cast<const f32x4*>(q) + v;
                *reinterpret_cast<f32x4*>(q) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gx + j < W) q[j] = accumulate ? q[j] + v[j] : v[j];
            }
        }
    }

    ssum = wave_sum(ssum);
    if (lane_id() == 0) red[t >> 6] = ssum;
    __syncthreads();
    if (t == 0) {
        float s = red[0];
#pragma unroll
        for (int k = 1; k < SS_TPB / 64; ++k) s += red[k];
        atomicAdd(loss, s / fN);
    }
}

}  // namespace

extern "C" int fw_ssim11_loss(const float* a, const float* b, float* da, int n, int C, int H, int W, float gscale, int accumulate,
                              float* loss, void* stream) {
    FW_CHECK_ARG(a && b && loss && n > 0 && C > 0);
    FW_CHECK_ARG(H >= 8 && H <= 1024 && W >= 8 && W <= 1024);
    const int tiles_x = fw_cdiv(W, SS_T), tiles_y = fw_cdiv(H, SS_T);
    const long blocks = (long)n * C * tiles_x * tiles_y;
    FW_CHECK_ARG(blocks <= 2147483647L);
    const double N = (double)n * C * H * W;
    const int vec = da && W % 4 == 0 && (reinterpret_cast<uintptr_t>(da) & 15) == 0;
    hipLaunchKernelGGL(ssim11_loss_kernel, dim3((unsigned)blocks), dim3(SS_TPB), 0, (hipStream_t)stream, a, b, da, H, W, tiles_x, tiles_y,
                       (float)((double)gscale / N), (float)N, accumulate, vec, loss);
    FW_LAUNCH_RET();
}
