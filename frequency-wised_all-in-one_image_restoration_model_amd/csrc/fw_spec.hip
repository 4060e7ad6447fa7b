// Band statistics of the 2-D spectrum of maps of ANY size: H x W with 8 <= H, W <= 1024 independent of each other (odd sides,
// W % 4 != 0 included).  out[image][band] = sum over the frequency bins of the band of |DFT2(map)| or |DFT2(map)|^2, the DFT
// un-normalised (utils/visualization_utils.py:158-184 get_frequency_distribution, and the per-band error energy of restore.py).
//
// The arithmetic is fw_dft.hip's: exact f32 products on v_mfma_f32_16x16x4_f32, f32 accumulation, both operands read as ready-made
// fragments through L2, a 64 x 64 output tile per workgroup (4 waves, 2 x 2), no LDS tile.  Two passes and a fold:
//     row pass      T^t[v][y] = sum_x src(y, x) W_W[x][v]        real in, complex out; the SOURCE is converted in the loader
//                                                                (f32 map, u8 map, or clamp(restored, 0, 1) - clean / 255)
//     column pass   F[u][v]   = sum_y T^t[v][y] W_H[y][u]        never written: the epilogue takes |F| or |F|^2, looks the bin's band
//                                                                up in ring[u][v] and reduces per band -> one f32 per (map, tile, band)
//     fold          out[n][b] = sum over the tiles, in tile order, in double
// Half the spectrum.  The maps are real, so |F[(H - u) % H][(W - v) % W]| = |F[u][v]|: both passes compute the columns v <= W / 2 only,
// and the epilogue adds a bin's value to the band of its mirror bin as well (looked up in the ring on its own -- the ring need not be
// symmetric) unless the bin is its own mirror column (v = 0, or 2 v = W).
// Edges.  Hp = 64 ceil(H / 64), Wp = 64 ceil(W / 64), Wh = 64 ceil((W / 2 + 1) / 64).  The panels come zero-filled to [3][Hp][Hp] and
// [3][Wp][Wp], T^t is [Wh][Hp]: every panel and work-buffer access is a whole in-bounds 16-byte piece.  The row pass writes ALL of
// T^t (a padded y meets zero data rows; the rows v > W / 2 of the last tile are computed or zero, and belong to no band), so the
// column pass reads only what the row pass wrote.  The caller's maps and ring have pitch W: their accesses are guarded per element
// (one 16-byte / 4-byte load where W % 4 == 0 and the base is aligned).  The contraction stops at the last 16-chunk that holds data
// (ceil(W / 16), ceil(H / 16)), not at the tile grid.
// No floating-point atomics anywhere: a band's sum over a wave is a fixed shuffle tree, over the workgroup a fixed four-term sum,
// over the tiles a fixed loop -- two runs on the same input give the same bits.
// fw_band_split, further down, goes on from the same row pass to the bands themselves: band images, masked spectra, magnitudes.
#include "fw_common.h"

namespace {

// Every pass below is a chunk loop over DftChunk (fw_common.h): data and panels loaded per 16-float chunk, single-buffered, then mac().

// KIND 0: f32 map; 1: u8 map; 2: clamp(restored f32, 0, 1) - clean u8 / 255 (the difference eval_blend_body squares, fw_data.hip)
template <int KIND> FW_DEV float spec_value(const float* f, const unsigned char* q, size_t i) {
    if (KIND == 0) return f[i];
    if (KIND == 1) return (float)q[i];
    return fminf(fmaxf(f[i], 0.f), 1.f) - __fdiv_rn((float)q[i], 255.0f);
}
// a lane's 4 consecutive x of row y, zero outside the map; vec: W % 4 == 0 and aligned bases, so x < W covers x + 3
template <int KIND> FW_DEV f32x4 spec_src_frag(const float* f, const unsigned char* q, int H, int W, int y, int x, bool vec) {
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (y >= H || x >= W) return r;
    const size_t i = (size_t)y * W + x;
    if (vec) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        unsigned char b[4] = {0, 0, 0, 0};
        if (KIND != 1) a = *reinterpret_cast<const f32x4*>(f + i);
        if (KIND != 0) *reinterpret_cast<unsigned*>(b) = *reinterpret_cast<const unsigned*>(q + i);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            r[k] = KIND == 0 ? a[k] : KIND == 1 ? (float)b[k] : fminf(fmaxf(a[k], 0.f), 1.f) - __fdiv_rn((float)b[k], 255.0f);
        return r;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (x + k < W) r[k] = spec_value<KIND>(f, q, i + k);
    return r;
}

FW_DEV int mirror_index(int n, int k) { return k ? n - k : 0; }             // (n - k) % n for k < n
// g: the band of the bin (u, v); gm: the band of its mirror bin ((H - u) % H, (W - v) % W), looked up on its own -- the ring need not be
// symmetric.  255: none (outside u < H, 2 v <= W; gm also in the bin's own mirror column, v = 0 or 2 v = W, unless own_column).
// T: spec_col_kernel takes bytes, whose compares in its band reduction then stay byte-wide (with int the kernel was measurably slower
// on one map, profiles/r16_dft_tile_meta.txt); spec_coli_kernel takes int.
template <typename T> FW_DEV void ring_pair(const unsigned char* ring, int H, int W, int u, int v, bool own_column, T& g, T& gm) {
    g = gm = 255;
    if (u >= H || 2 * v > W) return;
    g = ring[(size_t)u * W + v];
    if (own_column || (v != 0 && 2 * v != W)) gm = ring[(size_t)mirror_index(H, u) * W + mirror_index(W, v)];
}

// grid (Wh / 64 tiles of v, Hp / 64 tiles of y, nimg); 256 threads.  Tr, Ti: [nimg][Wh][Hp].
template <int KIND>
__global__ __launch_bounds__(256) void spec_row_kernel(const float* __restrict__ srcf, const unsigned char* __restrict__ srcq,
                                                       const float* __restrict__ PW, float* __restrict__ Tr, float* __restrict__ Ti, int H,
                                                       int W, int Hp, int Wp, int Wh, int vec) {
    const int w = threadIdx.x >> 6, l = lane_id();
    const size_t img = blockIdx.z;
    const int d0 = blockIdx.y * 64 + (w >> 1) * 32, p0 = blockIdx.x * 64 + (w & 1) * 32;
    const float* f = KIND == 1 ? nullptr : srcf + img * H * W;
    const unsigned char* q = KIND == 0 ? nullptr : srcq + img * H * W;
    f32x4 accr[2][2], acci[2][2];
    zero_acc(accr); zero_acc(acci);
    const int KC = (W + 15) / 16;
    for (int c = 0; c < KC; ++c) {
        DftChunk<true, false, false> ch;                                    // real in, W: -sin carries it into the imaginary output
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            ch.ar[t] = spec_src_frag<KIND>(f, q, H, W, d0 + 16 * t + (l & 15), c * 16 + ((l >> 4) << 2), vec != 0);
            ch.load_panels(t, PW, Wp, p0, c, false);
        }
        ch.mac(accr, acci);
    }
    // acc element r of lane l is out[m = data row y 4 (l >> 4) + r][n = panel row v l & 15]: the transpose takes one 16-byte store
    float* o_r = Tr + img * Wh * Hp;
    float* o_i = Ti + img * Wh * Hp;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const size_t o = (size_t)(p0 + 16 * nt + (l & 15)) * Hp + d0 + 16 * mt + ((l >> 4) << 2);
            *reinterpret_cast<f32x4*>(o_r + o) = accr[mt][nt];
            *reinterpret_cast<f32x4*>(o_i + o) = acci[mt][nt];
        }
}

// grid (Hp / 64 tiles of u, Wh / 64 tiles of v, nimg); 256 threads.  part: [nimg][tiles][nbands], tile = blockIdx.y * gridDim.x + blockIdx.x.
__global__ __launch_bounds__(256) void spec_col_kernel(const float* __restrict__ Tr, const float* __restrict__ Ti, const float* __restrict__ PH,
                                                       const unsigned char* __restrict__ ring, float* __restrict__ part, int H, int W,
                                                       int Hp, int Wh, int nbands, int power) {
    __shared__ float red[4][32];
    const int w = threadIdx.x >> 6, l = lane_id();
    const size_t img = blockIdx.z;
    const int d0 = blockIdx.y * 64 + (w >> 1) * 32, p0 = blockIdx.x * 64 + (w & 1) * 32;       // d: v (rows of T^t), p: u
    const float* xr = Tr + img * Wh * Hp;
    const float* xi = Ti + img * Wh * Hp;
    f32x4 accr[2][2], acci[2][2];
    zero_acc(accr); zero_acc(acci);
    const int KC = (H + 15) / 16;
    for (int c = 0; c < KC; ++c) {
        DftChunk<false, false, false> ch;                                   // (a + i b)(C - i S) = a C + b S + i (b C - a S)
        ch.load(xr, xi, Hp, d0, PH, Hp, p0, c, false);
        ch.mac(accr, acci);
    }
    // acc element r of lane l: v = d0 + 16 mt + 4 (l >> 4) + r, u = p0 + 16 nt + (l & 15)
    float val[16];
    unsigned char bnd[16], mir[16];                                        // the band of the bin, and of its mirror bin
    unsigned mine = 0u;                                                    // bands this lane holds a bin of
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = (nt * 2 + mt) * 4 + r;
                const int u = p0 + 16 * nt + (l & 15), v = d0 + 16 * mt + ((l >> 4) << 2) + r;
                const float a = accr[mt][nt][r], b = acci[mt][nt][r];
                const float e = a * a + b * b;
                val[k] = power ? e : sqrtf(e);
                unsigned char g, gm;                                        // bytes, as the table's: the compares below stay byte-wide
                ring_pair(ring, H, W, u, v, false, g, gm);                  // a bin in its own mirror column counts once
                if (g >= nbands) g = 255;
                if (gm >= nbands) gm = 255;
                bnd[k] = g; mir[k] = gm;
                if (g != 255) mine |= 1u << g;
                if (gm != 255) mine |= 1u << gm;
            }
    for (int b = 0; b < nbands; ++b) {                                      // uniform over the wave
        float s = 0.f;
        if (__any((mine >> b) & 1u)) {
#pragma unroll
            for (int k = 0; k < 16; ++k) s += (bnd[k] == b ? val[k] : 0.f) + (mir[k] == b ? val[k] : 0.f);
            s = wave_sum(s);
        }
        if (l == 0) red[w][b] = s;
    }
    __syncthreads();
    if (threadIdx.x < nbands) {
        const int b = threadIdx.x;
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x, tiles = (size_t)gridDim.x * gridDim.y;
        part[(img * tiles + tile) * nbands + b] = ((red[0][b] + red[1][b]) + red[2][b]) + red[3][b];
    }
}

// grid nimg; 64 threads, one per band
__global__ __launch_bounds__(64) void spec_fold_kernel(const float* __restrict__ part, double* __restrict__ out, int tiles, int nbands) {
    const int b = threadIdx.x;
    if (b >= nbands) return;
    const float* p = part + (size_t)blockIdx.x * tiles * nbands + b;
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s += (double)p[(size_t)t * nbands];
    out[(size_t)blockIdx.x * nbands + b] = s;
}

// ---- fw_band_split: the bands themselves.  The row pass above, then
//     forward column pass   F^t[v][u] = sum_y T^t[v][y] W_H[y][u]       the half spectrum, written ONCE per map ([Wh][Hp], u contiguous)
//     inverse column pass   G_b[y][v] = sum_u w_b[u][v] F[u][v] e^{+2 pi i u y / H}                 per band, [Hp][Wh], v contiguous
//     inverse row pass      out_b[y][x] = 1 / (H W) sum_{v <= W / 2} Re(G_b[y][v] e^{+2 pi i v x / W})
// w_b[u][v] = c_v / 2 ([ring[u][v] == b] + [ring[(H - u) % H][(W - v) % W] == b]) for u < H, v <= W / 2, and 0 elsewhere; c_v = 1 for v = 0
// and 2 v = W, 2 otherwise.  Only the real part of the inverse is kept, so the Hermitian part of M_b F -- which is ((M_b[k] + M_b[-k]) / 2)
// F[k] -- gives it exactly for ANY ring; of a Hermitian spectrum the columns v and W - v add up to twice the real part of one of
// them.  w_b is 0, 1/2, 1 or 2: the product w_b F is exact.  The weight is applied to the F fragment as it is loaded; NB bands share a
// workgroup's F and panel fragments.  Modes 1 and 2 need no inverse: spec_bins_kernel reads F^t (the mirror bin conjugated).
// Padding: F^t is zero for u >= H (zero panel rows) and w_b is zero for v > W / 2, so G_b is zero there and for y >= H; every pass writes
// the whole padded array the next one reads.

// grid (Hp / 64 tiles of u, Wh / 64 tiles of v, nimg); 256 threads.  Fr, Fi: [nimg][Wh][Hp].
__global__ __launch_bounds__(256) void spec_colf_kernel(const float* __restrict__ Tr, const float* __restrict__ Ti, const float* __restrict__ PH,
                                                        float* __restrict__ Fr, float* __restrict__ Fi, int H, int Hp, int Wh) {
    const int w = threadIdx.x >> 6, l = lane_id();
    const size_t img = blockIdx.z;
    const int d0 = blockIdx.y * 64 + (w >> 1) * 32, p0 = blockIdx.x * 64 + (w & 1) * 32;       // d: v (rows of T^t), p: u
    const float* xr = Tr + img * Wh * Hp;
    const float* xi = Ti + img * Wh * Hp;
    f32x4 accr[2][2], acci[2][2];
    zero_acc(accr); zero_acc(acci);
    const int KC = (H + 15) / 16;
    for (int c = 0; c < KC; ++c) {
        DftChunk<false, false, true> ch;                                    // the panel is the first operand: the accumulator's 4 rows are u
        ch.load(xr, xi, Hp, d0, PH, Hp, p0, c, false);
        ch.mac(accr, acci);
    }
    // acc element r of lane l: u = p0 + 16 mt + 4 (l >> 4) + r, v = d0 + 16 nt + (l & 15)
    float* o_r = Fr + img * Wh * Hp;
    float* o_i = Fi + img * Wh * Hp;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const size_t o = (size_t)(d0 + 16 * nt + (l & 15)) * Hp + p0 + 16 * mt + ((l >> 4) << 2);
            *reinterpret_cast<f32x4*>(o_r + o) = accr[mt][nt];
            *reinterpret_cast<f32x4*>(o_i + o) = acci[mt][nt];
        }
}

// grid (Hp / 64 tiles of y, Wh / 64 tiles of v, nimg); 256 threads.  The bands b0 .. b0 + NB - 1.  Gr, Gi: [NB][nimg][Hp][Wh].
template <int NB>
__global__ __launch_bounds__(256) void spec_coli_kernel(const float* __restrict__ Fr, const float* __restrict__ Fi, const float* __restrict__ PH,
                                                        const unsigned char* __restrict__ ring, float* __restrict__ Gr, float* __restrict__ Gi,
                                                        int H, int W, int Hp, int Wh, int b0) {
    const int w = threadIdx.x >> 6, l = lane_id();
    const size_t img = blockIdx.z, nimg = gridDim.z;
    const int d0 = blockIdx.y * 64 + (w >> 1) * 32, p0 = blockIdx.x * 64 + (w & 1) * 32;       // d: v (rows of F^t), p: y
    const float* xr = Fr + img * Wh * Hp;
    const float* xi = Fi + img * Wh * Hp;
    f32x4 accr[NB][2][2], acci[NB][2][2];
#pragma unroll
    for (int j = 0; j < NB; ++j) { zero_acc(accr[j]); zero_acc(acci[j]); }
    const int KC = (H + 15) / 16;
    for (int c = 0; c < KC; ++c) {
        DftChunk<false, false, false> ch;                                   // conj(W): (a + i b)(C + i S) = a C - b S + i (a S + b C)
        f32x4 fr[2], fi[2];                                                 // the F fragments every band of the group weights
        int g[2][4], gm[2][4];                                              // band of the bin and of its mirror bin, 255: weight 0
        float cv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            fr[t] = frag_g(xr, Hp, d0 + 16 * t, c);
            fi[t] = frag_g(xi, Hp, d0 + 16 * t, c);
            ch.load_panels(t, PH, Hp, p0, c, true);
            const int v = d0 + 16 * t + (l & 15);
            cv[t] = (v == 0 || 2 * v == W) ? 0.5f : 1.0f;                   // its own mirror column: both lookups, half the weight
#pragma unroll
            for (int s = 0; s < 4; ++s) ring_pair(ring, H, W, c * 16 + ((l >> 4) << 2) + s, v, true, g[t][s], gm[t][s]);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float wt = cv[t] * ((g[t][s] == b0 + j ? 1.f : 0.f) + (gm[t][s] == b0 + j ? 1.f : 0.f));
                    ch.ar[t][s] = wt * fr[t][s];
                    ch.ai[t][s] = wt * fi[t][s];
                }
            ch.mac(accr[j], acci[j]);
        }
    }
    // acc element r of lane l: v = d0 + 16 mt + 4 (l >> 4) + r, y = p0 + 16 nt + (l & 15)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        float* o_r = Gr + ((size_t)j * nimg + img) * Hp * Wh;
        float* o_i = Gi + ((size_t)j * nimg + img) * Hp * Wh;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const size_t o = (size_t)(p0 + 16 * nt + (l & 15)) * Wh + d0 + 16 * mt + ((l >> 4) << 2);
                *reinterpret_cast<f32x4*>(o_r + o) = accr[j][mt][nt];
                *reinterpret_cast<f32x4*>(o_i + o) = acci[j][mt][nt];
            }
    }
}

// grid (Wp / 64 tiles of x, Hp / 64 tiles of y times the bands of the group, nimg); 256 threads.  out: [.][nimg][H][W] from band b0 on.
__global__ __launch_bounds__(256) void spec_rowi_kernel(const float* __restrict__ Gr, const float* __restrict__ Gi, const float* __restrict__ PW,
                                                        float* __restrict__ out, int H, int W, int Hp, int Wp, int Wh, int b0, float scale,
                                                        int vec) {
    const int w = threadIdx.x >> 6, l = lane_id();
    const size_t img = blockIdx.z, nimg = gridDim.z;
    const int ty = blockIdx.y % (Hp / 64), j = blockIdx.y / (Hp / 64);
    const int d0 = ty * 64 + (w >> 1) * 32, p0 = blockIdx.x * 64 + (w & 1) * 32;               // d: y (rows of G), p: x
    const float* xr = Gr + ((size_t)j * nimg + img) * Hp * Wh;
    const float* xi = Gi + ((size_t)j * nimg + img) * Hp * Wh;
    f32x4 acc[2][2];
    zero_acc(acc);
    const int KC = (W / 2 + 1 + 15) / 16;
    for (int c = 0; c < KC; ++c) {
        DftChunk<false, true, true> ch;                                     // Re((a + i b)(C + i S)) = a C - b S; the panel first: 4 rows are x
        ch.load(xr, xi, Wh, d0, PW, Wp, p0, c, true);
        ch.mac(acc);
    }
    // acc element r of lane l: x = p0 + 16 mt + 4 (l >> 4) + r, y = d0 + 16 nt + (l & 15); vec: W % 4 == 0 and an aligned base
    float* o = out + ((size_t)(b0 + j) * nimg + img) * H * W;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int y = d0 + 16 * nt + (l & 15), x = p0 + 16 * mt + ((l >> 4) << 2);
            if (y >= H || x >= W) continue;
            f32x4 r = acc[mt][nt];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] *= scale;
            float* q = o + (size_t)y * W + x;
            if (vec) {
                *reinterpret_cast<f32x4*>(q) = r;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k < W) q[k] = r[k];
            }
        }
}

// Modes 1 and 2: one thread per element of the output plane.  grid (ceil(H W / 256), nimg); 256 threads.
// MODE 1: (re, im) of M_b F at [u][v]; MODE 2: |M_b F| at [(u + H / 2) % H][(v + W / 2) % W].
template <int MODE>
__global__ __launch_bounds__(256) void spec_bins_kernel(const float* __restrict__ Fr, const float* __restrict__ Fi,
                                                        const unsigned char* __restrict__ ring, float* __restrict__ out, int H, int W, int Hp,
                                                        int Wh, int nbands) {
    const size_t img = blockIdx.y, nimg = gridDim.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    int u = i / W, v = i - u * W;
    if (MODE == 2) {                                                        // the output element (u, v) shows the bin (u - H / 2, v - W / 2)
        u -= H / 2; if (u < 0) u += H;
        v -= W / 2; if (v < 0) v += W;
    }
    const int g = ring[(size_t)u * W + v];
    const bool half = 2 * v <= W;                                           // else the mirror bin, conjugated
    const size_t f = img * Wh * Hp + (size_t)(half ? v : mirror_index(W, v)) * Hp + (half ? u : mirror_index(H, u));
    const float re = Fr[f], im = half ? Fi[f] : -Fi[f];
    const float mag = sqrtf(re * re + im * im);
    for (int b = 0; b < nbands; ++b) {
        const size_t o = ((size_t)b * nimg + img) * H * W + i;
        const bool in = g == b;
        if (MODE == 1) *reinterpret_cast<float2*>(out + 2 * o) = make_float2(in ? re : 0.f, in ? im : 0.f);
        else out[o] = in ? mag : 0.f;
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

// What fw_band_stats and fw_band_split share: the argument checks, the padded geometry, the source as the row pass reads it
// (vec: W % 4 == 0 and aligned bases) and per, the floats of one [nimg][Wh][Hp] work array.
struct SpecGeom { int Hp, Wp, Wh, vec; size_t per; const float* f; const unsigned char* q; };
static int spec_geom(SpecGeom& g, int src_kind, const void* src, const unsigned char* clean, const float* panels_h, const float* panels_w,
                     const float* work, int nimg, int H, int W, int nbands) {
    FW_CHECK_ARG(src && panels_h && panels_w && work && src_kind >= 0 && src_kind <= 2 && (src_kind != 2 || clean) && nimg > 0 &&
                 nimg <= 65535 && H >= 8 && H <= 1024 && W >= 8 && W <= 1024 && nbands >= 1 && nbands <= 32);
    FW_CHECK_ARG((((uintptr_t)panels_h | (uintptr_t)panels_w | (uintptr_t)work) & 15) == 0 && (src_kind == 1 || ((uintptr_t)src & 3) == 0));
    g.Hp = (H + 63) / 64 * 64; g.Wp = (W + 63) / 64 * 64; g.Wh = (W / 2 + 1 + 63) / 64 * 64;
    g.per = (size_t)nimg * g.Hp * g.Wh;
    g.f = src_kind == 1 ? nullptr : (const float*)src;
    g.q = src_kind == 1 ? (const unsigned char*)src : clean;
    g.vec = W % 4 == 0 && (!g.f || ((uintptr_t)g.f & 15) == 0) && (!g.q || ((uintptr_t)g.q & 3) == 0);
    return 0;
}
static void spec_launch_row(const SpecGeom& g, int src_kind, const float* panels_w, float* Tr, float* Ti, int nimg, int H, int W, void* stream) {
#define SPEC_ROW(KIND)                                                                                                              \
    hipLaunchKernelGGL(spec_row_kernel<KIND>, dim3(g.Wh / 64, g.Hp / 64, nimg), dim3(256), 0, ST, g.f, g.q, panels_w, Tr, Ti, H, W, g.Hp, \
                       g.Wp, g.Wh, g.vec)
    if (src_kind == 0) SPEC_ROW(0); else if (src_kind == 1) SPEC_ROW(1); else SPEC_ROW(2);
#undef SPEC_ROW
}

extern "C" int fw_band_stats(int src_kind, const void* src, const unsigned char* clean, const unsigned char* ring, const float* panels_h,
                             const float* panels_w, float* work, double* out, int nimg, int H, int W, int nbands, int power, void* stream) {
    SpecGeom g;
    const int rc = spec_geom(g, src_kind, src, clean, panels_h, panels_w, work, nimg, H, W, nbands);
    if (rc) return rc;
    FW_CHECK_ARG(ring && out && (power == 0 || power == 1) && ((uintptr_t)out & 7) == 0);
    const int Hp = g.Hp, Wh = g.Wh, tiles = (Hp / 64) * (Wh / 64);
    float* Tr = work; float* Ti = work + g.per; float* part = work + 2 * g.per;
    spec_launch_row(g, src_kind, panels_w, Tr, Ti, nimg, H, W, stream);
    hipLaunchKernelGGL(spec_col_kernel, dim3(Hp / 64, Wh / 64, nimg), dim3(256), 0, ST, Tr, Ti, panels_h, ring, part, H, W, Hp, Wh, nbands, power);
    hipLaunchKernelGGL(spec_fold_kernel, dim3(nimg), dim3(64), 0, ST, part, out, tiles, nbands);
    FW_LAUNCH_RET();
}

extern "C" int fw_band_split(int src_kind, const void* src, const unsigned char* clean, const unsigned char* ring, const float* panels_h,
                             const float* panels_w, float* work, float* out, int nimg, int H, int W, int nbands, int mode, void* stream) {
    SpecGeom g;
    const int rc = spec_geom(g, src_kind, src, clean, panels_h, panels_w, work, nimg, H, W, nbands);
    if (rc) return rc;
    FW_CHECK_ARG(ring && out && mode >= 0 && mode <= 2 && ((uintptr_t)out & (mode == 1 ? 7 : 3)) == 0);
    const int Hp = g.Hp, Wp = g.Wp, Wh = g.Wh;
    const size_t per = g.per;
    float* Tr = work; float* Ti = work + per; float* Fr = work + 2 * per; float* Fi = work + 3 * per;
    const dim3 gcol(Hp / 64, Wh / 64, nimg);
    spec_launch_row(g, src_kind, panels_w, Tr, Ti, nimg, H, W, stream);
    hipLaunchKernelGGL(spec_colf_kernel, gcol, dim3(256), 0, ST, Tr, Ti, panels_h, Fr, Fi, H, Hp, Wh);
    if (mode != 0) {
        const dim3 gb((H * W + 255) / 256, nimg);
        if (mode == 1) hipLaunchKernelGGL(spec_bins_kernel<1>, gb, dim3(256), 0, ST, Fr, Fi, ring, out, H, W, Hp, Wh, nbands);
        else hipLaunchKernelGGL(spec_bins_kernel<2>, gb, dim3(256), 0, ST, Fr, Fi, ring, out, H, W, Hp, Wh, nbands);
        FW_LAUNCH_RET();
    }
    // up to 4 bands at a time share the F and panel fragments of a workgroup; the group's G is reused by the next group (stream order)
    const int NBG = nbands < 4 ? nbands : 4;
    float* Gr = work + 4 * per; float* Gi = Gr + (size_t)NBG * nimg * Hp * Wh;
    const int ovec = W % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const float scale = 1.0f / ((float)H * (float)W);
    for (int b0 = 0; b0 < nbands; b0 += 4) {
        const int nb = nbands - b0 < 4 ? nbands - b0 : 4;
#define SPEC_COLI(NB) hipLaunchKernelGGL(spec_coli_kernel<NB>, gcol, dim3(256), 0, ST, Fr, Fi, panels_h, ring, Gr, Gi, H, W, Hp, Wh, b0)
        if (nb == 1) SPEC_COLI(1); else if (nb == 2) SPEC_COLI(2); else if (nb == 3) SPEC_COLI(3); else SPEC_COLI(4);
#undef SPEC_COLI
        hipLaunchKernelGGL(spec_rowi_kernel, dim3(Wp / 64, (Hp / 64) * nb, nimg), dim3(256), 0, ST, Gr, Gi, panels_w, out, H, W, Hp, Wp, Wh, b0,
                           scale, ovec);
    }
    FW_LAUNCH_RET();
}
