// Callers either side of the model as device kernels, so that neither the input pipeline nor the evaluation
// bounds the training rate:
//   * fw_train_batch  -- one launch makes a whole training batch from uint8 images resident in HBM: Gaussian noise synthesis on the
//     uint8 grid (utils/dataset_utils.py:122-126), two independent random crops of the SAME degraded image (:131-132, `_crop_patch`),
//     one of the 7 flip / rotation modes per crop (utils/image_utils.py:133-182 `random_augmentation`), ToTensor scaling (:134-135).
//     No host round trip: crop origins and modes come from one device tensor of random integers, the noise is counter-based
//     (fw_common.h hash -> Box-Muller), so both crops see the same noisy image although that image is never materialised.
//   * fw_train_batch_synth -- the same batch with rain, haze and motion blur synthesised per slot in the launch (integer arithmetic on two
//     small tables, fresh per batch, one degraded image for both crops of a sample); fw_synth_image writes that image out for inspection.
//     Stand-ins for the paired training sets, not models of them.
//   * fw_tile_gather / fw_tile_blend -- test.py:47-71: cut a test image into tiles (stride = tile, last tile flush with the border),
//     and average the RESTORED tiles over their overlap (gather form: at most two tiles per axis cover a pixel; no atomics).
//   * fw_ssim7 -- structural similarity as utils/val_utils.py:50-66 calls it (skimage.metrics.structural_similarity defaults: 7x7
//     uniform window, K1 = 0.01, K2 = 0.03, sample covariance, border of 3 pixels cropped, mean over channels), inputs clipped to [0, 1].
//   * fw_eval_gather / fw_eval_blend / fw_eval_ssim7 -- the same three steps for a whole CHUNK of test images of different sizes in one
//     launch each, driven by tables in HBM (fwair/evaluate.py EvalEngine): tiles straight from the uint8 images (paired test sets) or
//     with the test set's Gaussian noise synthesised on the fly (utils/dataset_utils.py:177-182; same counter-based draw as
//     fw_train_batch, so overlapping tiles see one noisy image that is never stored); the overlap average into a packed f32 buffer
//     together with the squared error against the ground truth (utils/val_utils.py:52-63) and the uint8 image of utils/image_io.py:383;
//     SSIM over the packed buffer.  Four consecutive x per thread (one 4-byte load of uint8 / one 16-byte access of f32) where the
//     row pitch and the pointers are multiples of 4, one x per thread otherwise.
//   * fw_restore_gather / fw_restore_blend -- the same pair for images of ANY size: tiles may leave the image (whole-sample reflection,
//     np.pad 'reflect'), overlap by a chosen amount (a linear ramp weights the overlap) and come in the 8 flips / rotations of
//     fw_train_batch, which the blend undoes before it averages (x8 self-ensemble).  The noise counter is the SOURCE pixel, so
//     reflected copies, overlapping tiles and all eight turns see one noisy image.
// All HBM-bound byte / float streaming work: grid-stride kernels, coalesced along x.
#include "fw_common.h"

namespace {
constexpr int TPB = 256;
FW_DEV long gtid() { return (long)blockIdx.x * blockDim.x + threadIdx.x; }
FW_DEV long gstride() { return (long)gridDim.x * blockDim.x; }
static inline int grid_for(long n) { long g = (n + TPB - 1) / TPB; return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g)); }

// ---- training batch ---------------------------------------------------------------------------------------------------------------
// tab[b] = {clean ptr (u8 [3][H][W]), degraded ptr (u8, same shape) or 0, H, W};  rnd[b] = {ry1, rx1, rm1, ry2, rx2, rm2} >= 0
// out: d1, d2, c1, c2 f32 [B][3][S][S].   sigma[b]: noise level when no degraded image is given (0: the clean image itself).
__global__ void train_batch_kernel(const long long* __restrict__ tab, const int* __restrict__ rnd, const float* __restrict__ sigma,
                                   const unsigned* __restrict__ seed, unsigned site, float* __restrict__ d1, float* __restrict__ d2,
                                   float* __restrict__ c1, float* __restrict__ c2, int B, int S) {
    const long per = (long)3 * S * S, n = (long)B * 2 * per;
    for (long i = gtid(); i < n; i += gstride()) {
        const int ox = (int)(i % S), oy = (int)((i / S) % S), c = (int)((i / ((long)S * S)) % 3);
        const int v = (int)((i / per) % 2), b = (int)(i / (2 * per));
        const unsigned char* clean = reinterpret_cast<const unsigned char*>(tab[b * 4 + 0]);
        const unsigned char* degr = reinterpret_cast<const unsigned char*>(tab[b * 4 + 1]);
        const int H = (int)tab[b * 4 + 2], W = (int)tab[b * 4 + 3];
        const int* r = rnd + b * 6 + v * 3;
        const int y0 = r[0] % (H - S + 1), x0 = r[1] % (W - S + 1), mode = 1 + r[2] % 7;
        const int k = mode >> 1, ii = (mode & 1) ? S - 1 - oy : oy, jj = ox;          // flipud last -> undone first
        int py, px;
        if (k == 0) { py = ii; px = jj; }
        else if (k == 1) { py = jj; px = S - 1 - ii; }
        else if (k == 2) { py = S - 1 - ii; px = S - 1 - jj; }
        else { py = S - 1 - jj; px = ii; }
        const long pi = ((long)c * H + (y0 + py)) * W + (x0 + px);
        const float g = (float)clean[pi];
        float d;
        if (degr) d = (float)degr[pi];
        else {
            const float sg = sigma[b];
            d = g;
            if (sg > 0.f) {
                const unsigned key = fw_site_key(seed[0], site + (unsigned)b);
                const unsigned r1 = fw_hash32((unsigned)pi ^ key), r2 = fw_hash32(r1 + 0x9E3779B9U);
                const float u1 = ((float)r1 + 1.0f) * 2.3283064365386963e-10f, u2 = (float)r2 * 2.3283064365386963e-10f;
                const float z = sqrtf(-2.0f * __logf(u1)) * __cosf(6.283185307179586f * u2);
                d = floorf(fminf(fmaxf(g + z * sg, 0.f), 255.f));                     // clip, then astype(uint8) truncates
            }
        }
        const long o = ((long)b * 3 + c) * S * S + (long)oy * S + ox;
        (v ? d2 : d1)[o] = __fdiv_rn(d, 255.0f);                                 // ToTensor divides (correctly rounded), bit-exact with numpy
        (v ? c2 : c1)[o] = __fdiv_rn(g, 255.0f);
    }
}

// ---- evaluation tiles -------------------------------------------------------------------------------------------------------------
__global__ void tile_gather_kernel(const float* __restrict__ img, const int* __restrict__ ys, const int* __restrict__ xs, float* __restrict__ tiles,
                                   int C, int H, int W, int ny, int nx, int T) {
    const long n = (long)ny * nx * C * T * T;
    for (long i = gtid(); i < n; i += gstride()) {
        const int j = (int)(i % T), ii = (int)((i / T) % T), c = (int)((i / ((long)T * T)) % C), t = (int)(i / ((long)T * T * C));
        tiles[i] = img[((long)c * H + ys[t / nx] + ii) * W + xs[t % nx] + j];
    }
}
__global__ void tile_blend_kernel(const float* __restrict__ tiles, const int* __restrict__ ys, const int* __restrict__ xs, float* __restrict__ out,
                                  int C, int H, int W, int ny, int nx, int T) {
    const long n = (long)C * H * W;
    for (long i = gtid(); i < n; i += gstride()) {
        const int x = (int)(i % W), y = (int)((i / W) % H), c = (int)(i / ((long)W * H));
        float acc = 0.f, cnt = 0.f;
        for (int a = 0; a < ny; ++a) {
            const int dy = y - ys[a];
            if (dy < 0 || dy >= T) continue;
            for (int b = 0; b < nx; ++b) {
                const int dx = x - xs[b];
                if (dx < 0 || dx >= T) continue;
                acc += tiles[(((long)(a * nx + b) * C + c) * T + dy) * T + dx];
                cnt += 1.f;
            }
        }
        out[i] = acc / cnt;
    }
}

// ---- SSIM -------------------------------------------------------------------------------------------------------------------------
// a, b: f32 [n][C][H][W]; out[i] += sum over (c, interior y, x) of the SSIM map of image i (the caller divides by C (H-6) (W-6))
__global__ void ssim7_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int n, int C, int H, int W) {
    __shared__ float red[TPB / 64];
    const int hh = H - 6, ww = W - 6;
    const long per = (long)C * hh * ww;
    const int img = blockIdx.y;
    float acc = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % ww), y = (int)((i / ww) % hh), c = (int)(i / ((long)ww * hh));
        const float* pa = a + (((long)img * C + c) * H + y) * W + x;
        const float* pb = b + (((long)img * C + c) * H + y) * W + x;
        float sa = 0.f, sb = 0.f, saa = 0.f, sbb = 0.f, sab = 0.f;
        for (int dy = 0; dy < 7; ++dy)
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) {
                const float u = fminf(fmaxf(pa[dy * W + dx], 0.f), 1.f), v = fminf(fmaxf(pb[dy * W + dx], 0.f), 1.f);
                sa += u; sb += v; saa += u * u; sbb += v * v; sab += u * v;
            }
        const float inv = 1.0f / 49.0f, cn = 49.0f / 48.0f;
        const float ua = sa * inv, ub = sb * inv;
        const float va = cn * (saa * inv - ua * ua), vb = cn * (sbb * inv - ub * ub), vab = cn * (sab * inv - ua * ub);
        const float C1 = 1e-4f, C2 = 9e-4f;
        acc += ((2.f * ua * ub + C1) * (2.f * vab + C2)) / ((ua * ua + ub * ub + C1) * (va + vb + C2));
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < TPB / 64; ++i) s += red[i];
        atomicAdd(out + img, s);
    }
}

// ---- batched evaluation (a chunk of images per launch) ----------------------------------------------------------------------------
// itab[i] = {clean u8 ptr [3][H][W] or 0, degraded u8 ptr or 0, H, W};  ttab[t] = {image, y0, x0, 0};  gtab[i] = {offset of the image
// in the packed buffer (elements), first tile of the image in the chunk's tile buffer, ny, nx}
FW_DEV float noisy_u8(float g, float sg, unsigned key, long pi) {                     // train_batch_kernel's draw, same arithmetic
    const unsigned r1 = fw_hash32((unsigned)pi ^ key), r2 = fw_hash32(r1 + 0x9E3779B9U);
    const float u1 = ((float)r1 + 1.0f) * 2.3283064365386963e-10f, u2 = (float)r2 * 2.3283064365386963e-10f;
    const float z = sqrtf(-2.0f * __logf(u1)) * __cosf(6.283185307179586f * u2);
    return floorf(fminf(fmaxf(g + z * sg, 0.f), 255.f));
}
template <int V>
FW_DEV void eval_gather_body(const unsigned char* __restrict__ src, bool synth, float sg, unsigned key, float* __restrict__ out, int H, int W,
                             int y0, int x0, int T) {
    const int q = T / V, n = 3 * T * q;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += gridDim.x * blockDim.x) {
        const int j = (g % q) * V, i = (g / q) % T, c = g / (q * T);
        const long pi = ((long)c * H + (y0 + i)) * W + (x0 + j);
        unsigned char v[V];
        if constexpr (V == 4) *reinterpret_cast<unsigned*>(v) = *reinterpret_cast<const unsigned*>(src + pi);
        else v[0] = src[pi];
        float o[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float d = (float)v[k];
            if (synth) d = noisy_u8(d, sg, key, pi + k);
            o[k] = __fdiv_rn(d, 255.0f);
        }
        float* dst = out + ((long)c * T + i) * T + j;
        if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        else dst[0] = o[0];
    }
}
__global__ void eval_gather_kernel(const long long* __restrict__ itab, const int* __restrict__ ttab, const float* __restrict__ sigma,
                                   const unsigned* __restrict__ seed, unsigned site, float* __restrict__ tiles, int T) {
    const int t = blockIdx.y;
    const int im = ttab[t * 4 + 0], y0 = ttab[t * 4 + 1], x0 = ttab[t * 4 + 2];
    const unsigned char* clean = reinterpret_cast<const unsigned char*>(itab[im * 4 + 0]);
    const unsigned char* degr = reinterpret_cast<const unsigned char*>(itab[im * 4 + 1]);
    const int H = (int)itab[im * 4 + 2], W = (int)itab[im * 4 + 3];
    const unsigned char* src = degr ? degr : clean;
    if (!src || y0 < 0 || x0 < 0 || y0 + T > H || x0 + T > W) return;              // a tile outside its image is never read
    const float sg = sigma[im];
    const bool synth = !degr && sg > 0.f;
    const unsigned key = fw_site_key(seed[0], site + (unsigned)im);
    float* out = tiles + (long)t * 3 * T * T;
    if ((((long)src | W | x0) & 3) == 0) eval_gather_body<4>(src, synth, sg, key, out, H, W, y0, x0, T);
    else eval_gather_body<1>(src, synth, sg, key, out, H, W, y0, x0, T);
}

FW_DEV float block_sum(float acc, float* red) {                                        // valid on thread 0
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0)
        for (int i = 0; i < TPB / 64; ++i) s += red[i];
    return s;
}
template <int V>
FW_DEV float eval_blend_body(const unsigned char* __restrict__ clean, const int* __restrict__ ttab, const float* __restrict__ rest,
                             float* __restrict__ packed, unsigned char* __restrict__ u8out, int H, int W, int t0, int ny, int nx, int ntiles, int T) {
    const int wq = W / V;
    const long n = (long)3 * H * wq;
    float sse = 0.f;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long)gridDim.x * blockDim.x) {
        const int x = (int)(g % wq) * V, y = (int)((g / wq) % H), c = (int)(g / ((long)wq * H));
        // at most two tiles per axis cover a pixel: the regular one it falls into and the last one, flush with the border (test.py:48-49)
        const int a0 = min(y / T, ny - 1), b0 = min(x / T, nx - 1);
        float acc[V], cnt = 0.f;
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.f;
        for (int a = a0; a < ny; a += max(ny - 1 - a0, 1)) {
            for (int b = b0; b < nx; b += max(nx - 1 - b0, 1)) {
                const int ti = t0 + a * nx + b;
                if (ti >= ntiles) continue;
                const int dy = y - ttab[ti * 4 + 1], dx = x - ttab[ti * 4 + 2];
                if (dy < 0 || dy >= T || dx < 0 || dx >= T) continue;
                const float* p = rest + (((long)ti * 3 + c) * T + dy) * T + dx;
                if constexpr (V == 4) {
                    const float4 r = *reinterpret_cast<const float4*>(p);
                    acc[0] += r.x; acc[1 % V] += r.y; acc[2 % V] += r.z; acc[3 % V] += r.w;
                } else acc[0] += p[0];
                cnt += 1.f;
            }
        }
        const long pi = ((long)c * H + y) * W + x;
        float o[V];
        unsigned char gt[V], q[V];
        if (clean) {
            if constexpr (V == 4) *reinterpret_cast<unsigned*>(gt) = *reinterpret_cast<const unsigned*>(clean + pi);
            else gt[0] = clean[pi];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            o[k] = acc[k] / cnt;
            if (clean) {
                const float d = fminf(fmaxf(o[k], 0.f), 1.f) - __fdiv_rn((float)gt[k], 255.0f);
                sse += d * d;
            }
            q[k] = (unsigned char)fminf(fmaxf(o[k] * 255.0f, 0.f), 255.f);           // image_io.py:383: clip, astype(uint8) truncates
        }
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(packed + pi) = make_float4(o[0], o[1 % V], o[2 % V], o[3 % V]);
            if (u8out) *reinterpret_cast<unsigned*>(u8out + pi) = *reinterpret_cast<const unsigned*>(q);
        } else {
            packed[pi] = o[0];
            if (u8out) u8out[pi] = q[0];
        }
    }
    return sse;
}
__global__ void eval_blend_kernel(const long long* __restrict__ itab, const long long* __restrict__ gtab, const int* __restrict__ ttab,
                                  const float* __restrict__ rest, float* __restrict__ packed, unsigned char* __restrict__ u8out,
                                  float* __restrict__ sse, int i0, int ntiles, int T) {
    __shared__ float red[TPB / 64];
    const int im = i0 + blockIdx.y;
    const unsigned char* clean = reinterpret_cast<const unsigned char*>(itab[im * 4 + 0]);
    const int H = (int)itab[im * 4 + 2], W = (int)itab[im * 4 + 3];
    const long off = gtab[im * 4 + 0];
    const int t0 = (int)gtab[im * 4 + 1], ny = (int)gtab[im * 4 + 2], nx = (int)gtab[im * 4 + 3];
    float* pk = packed + off;
    unsigned char* u8 = u8out ? u8out + off : nullptr;
    float acc;
    if ((((long)clean | (long)u8 | off | W) & 3) == 0 && ((long)pk & 15) == 0)       // tile origins are then multiples of 4 too (T % 4 == 0)
        acc = eval_blend_body<4>(clean, ttab, rest, pk, u8, H, W, t0, ny, nx, ntiles, T);
    else
        acc = eval_blend_body<1>(clean, ttab, rest, pk, u8, H, W, t0, ny, nx, ntiles, T);
    if (!clean) return;
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) atomicAdd(sse + im, acc);
}

// ssim7_kernel's arithmetic, a = packed restored image (f32), b = clean uint8 / 255; four neighbouring windows per thread share their
// 7 x 10 pixels (each window still sums its 49 taps in ssim7_kernel's order).  out[image] += sum of the SSIM map.
__global__ void eval_ssim7_kernel(const long long* __restrict__ itab, const long long* __restrict__ gtab, const float* __restrict__ packed,
                                  float* __restrict__ out, int i0) {
    __shared__ float red[TPB / 64];
    const int im = i0 + blockIdx.y;
    const unsigned char* clean = reinterpret_cast<const unsigned char*>(itab[im * 4 + 0]);
    const int H = (int)itab[im * 4 + 2], W = (int)itab[im * 4 + 3];
    if (!clean || H < 7 || W < 7) return;
    const float* a = packed + gtab[im * 4 + 0];
    const int hh = H - 6, ww = W - 6, wq = (ww + 3) / 4;
    const long n = (long)3 * hh * wq;
    float acc = 0.f;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long)gridDim.x * blockDim.x) {
        const int x = (int)(g % wq) * 4, y = (int)((g / wq) % hh), c = (int)(g / ((long)wq * hh));
        float s[4][5];
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int k = 0; k < 5; ++k) s[o][k] = 0.f;
        for (int dy = 0; dy < 7; ++dy) {
            const long row = ((long)c * H + y + dy) * W + x;
            float u[10], v[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                const bool in = x + k < W;
                u[k] = in ? fminf(fmaxf(a[row + k], 0.f), 1.f) : 0.f;
                v[k] = in ? __fdiv_rn((float)clean[row + k], 255.0f) : 0.f;
            }
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int dx = 0; dx < 7; ++dx) {
                    const float uu = u[o + dx], vv = v[o + dx];
                    s[o][0] += uu; s[o][1] += vv; s[o][2] += uu * uu; s[o][3] += vv * vv; s[o][4] += uu * vv;
                }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (x + o >= ww) continue;
            const float inv = 1.0f / 49.0f, cn = 49.0f / 48.0f;
            const float ua = s[o][0] * inv, ub = s[o][1] * inv;
            const float va = cn * (s[o][2] * inv - ua * ua), vb = cn * (s[o][3] * inv - ub * ub), vab = cn * (s[o][4] * inv - ua * ub);
            const float C1 = 1e-4f, C2 = 9e-4f;
            acc += ((2.f * ua * ub + C1) * (2.f * vab + C2)) / ((ua * ua + ub * ub + C1) * (va + vb + C2));
        }
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) atomicAdd(out + im, acc);
}

// ---- restoration of any image size: reflect padding, weighted overlap, the eight turns --------------------------------------------
// ttab[t] = {image, y0, x0, mode}: [y0, y0 + T) / [x0, x0 + T) may leave the image, mode 0..7 turns the tile as train_batch_kernel's
// modes do.  gtab[i] = {packed offset, first tile, ny, nx, stride, nmodes, 0, 0}: tile (a, b, m) of the image is first + (a nx + b) nmodes + m.
// np.pad(mode='reflect') continued periodically ('edge' at n = 1): always inside [0, n)
FW_DEV int reflect_idx(int y, int n) {
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    int m = y % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}
// tile (oy, ox) -> where it comes from in the unturned tile (train_batch_kernel's map: flipud last -> undone first)
FW_DEV void mode_preimage(int mode, int T, int oy, int ox, int& py, int& px) {
    const int k = mode >> 1, ii = (mode & 1) ? T - 1 - oy : oy, jj = ox;
    if (k == 0) { py = ii; px = jj; }
    else if (k == 1) { py = jj; px = T - 1 - ii; }
    else if (k == 2) { py = T - 1 - ii; px = T - 1 - jj; }
    else { py = T - 1 - jj; px = ii; }
}
// its inverse: unturned (py, px) -> where the turned tile holds it
FW_DEV void mode_image(int mode, int T, int py, int px, int& oy, int& ox) {
    const int k = mode >> 1;
    int ii;
    if (k == 0) { ii = py; ox = px; }
    else if (k == 1) { ox = py; ii = T - 1 - px; }
    else if (k == 2) { ii = T - 1 - py; ox = T - 1 - px; }
    else { ox = T - 1 - py; ii = px; }
    oy = (mode & 1) ? T - 1 - ii : ii;
}
// One tile per blockIdx.y.  Stores run along ox in every mode.  Modes 0..1 and 4..5 (k = 0, 2) of a tile whose columns stay inside the
// image read four source bytes at once (reversed for k = 2); every other tile reads single bytes of the uint8 image, which for the
// transposing modes walks down a column: the image is a quarter of the tiles' bytes and stays in cache over its 8 turns.
__global__ void restore_gather_kernel(const long long* __restrict__ itab, const int* __restrict__ ttab, const float* __restrict__ sigma,
                                      const unsigned* __restrict__ seed, unsigned site, float* __restrict__ tiles, int T) {
    const int t = blockIdx.y;
    const int im = ttab[t * 4 + 0], y0 = ttab[t * 4 + 1], x0 = ttab[t * 4 + 2], mode = ttab[t * 4 + 3] & 7;
    const unsigned char* clean = reinterpret_cast<const unsigned char*>(itab[im * 4 + 0]);
    const unsigned char* degr = reinterpret_cast<const unsigned char*>(itab[im * 4 + 1]);
    const int H = (int)itab[im * 4 + 2], W = (int)itab[im * 4 + 3];
    const unsigned char* src = degr ? degr : clean;
    if (!src || H < 1 || W < 1) return;
    const float sg = sigma[im];
    const bool synth = !degr && sg > 0.f;
    const unsigned key = fw_site_key(seed[0], site + (unsigned)im);
    float* out = tiles + (long)t * 3 * T * T;
    const int k = mode >> 1;
    if ((k & 1) == 0 && x0 >= 0 && x0 + T <= W && (((long)src | W | x0) & 3) == 0) {
        const int q = T / 4, n = 3 * T * q;
        for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += gridDim.x * blockDim.x) {
            const int ox = (g % q) * 4, oy = (g / q) % T, c = g / (q * T);
            int py, px;
            mode_preimage(mode, T, oy, k ? ox + 3 : ox, py, px);                    // px: the lowest of the four source columns
            const long pi = ((long)c * H + reflect_idx(y0 + py, H)) * W + (x0 + px);
            unsigned char v[4];
            *reinterpret_cast<unsigned*>(v) = *reinterpret_cast<const unsigned*>(src + pi);
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float d = (float)v[e];
                if (synth) d = noisy_u8(d, sg, key, pi + e);
                o[e] = __fdiv_rn(d, 255.0f);
            }
            *reinterpret_cast<float4*>(out + ((long)c * T + oy) * T + ox) = k ? make_float4(o[3], o[2], o[1], o[0]) : make_float4(o[0], o[1], o[2], o[3]);
        }
        return;
    }
    const int n = 3 * T * T;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += gridDim.x * blockDim.x) {
        const int ox = g % T, oy = (g / T) % T, c = g / (T * T);
        int py, px;
        mode_preimage(mode, T, oy, ox, py, px);
        const long pi = ((long)c * H + reflect_idx(y0 + py, H)) * W + reflect_idx(x0 + px, W);   // the SOURCE pixel: also the noise counter
        float d = (float)src[pi];
        if (synth) d = noisy_u8(d, sg, key, pi);
        out[g] = __fdiv_rn(d, 255.0f);
    }
}

FW_DEV float ramp_weight(int i, int T, int ramp) { return __fdiv_rn((float)min(min(i + 1, T - i), ramp), (float)ramp); }
// V = 4: four consecutive x per thread; every tile origin of the image is then a multiple of 4, so the four lie in the same tiles.
// A tile of k = 0 / 2 holds them in one 16-byte word (reversed for k = 2); a transposing tile holds them down a column of the tile.
template <int V>
FW_DEV float restore_blend_body(const unsigned char* __restrict__ clean, const int* __restrict__ ttab, const float* __restrict__ rest,
                                float* __restrict__ packed, unsigned char* __restrict__ u8out, int H, int W, int t0, int ny, int nx, int stride,
                                int nmodes, int ntiles, int T, int ramp) {
    const int wq = W / V;
    const long n = (long)3 * H * wq;
    float sse = 0.f;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long)gridDim.x * blockDim.x) {
        const int x = (int)(g % wq) * V, y = (int)((g / wq) % H), c = (int)(g / ((long)wq * H));
        // regular tiles a stride <= y < a stride + T (a <= ny - 2), then the last one; the same along x: ascending tile order
        const int a0 = y < T ? 0 : (y - T) / stride + 1, a1 = min(y / stride, ny - 2);
        const int b0 = x < T ? 0 : (x - T) / stride + 1, b1 = min(x / stride, nx - 2);
        float acc[V], wsum[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = wsum[e] = 0.f;
        for (int a = a0; a < ny; a = (a < a1 ? a + 1 : (a < ny - 1 ? ny - 1 : ny))) {
            for (int b = b0; b < nx; b = (b < b1 ? b + 1 : (b < nx - 1 ? nx - 1 : nx))) {
                const long tb = (long)t0 + ((long)a * nx + b) * nmodes;
                if (tb < 0 || tb + nmodes > ntiles) continue;
                const int dy = y - ttab[tb * 4 + 1], dx = x - ttab[tb * 4 + 2];
                if (dy < 0 || dy >= T || dx < 0 || dx + V > T) continue;
                const float wy = ramp_weight(dy, T, ramp);
                float w[V];
#pragma unroll
                for (int e = 0; e < V; ++e) w[e] = __fmul_rn(wy, ramp_weight(dx + e, T, ramp));
                for (int m = 0; m < nmodes; ++m) {
                    const int mode = ttab[(tb + m) * 4 + 3] & 7;
                    const float* p = rest + ((tb + m) * 3 + c) * T * T;
                    int oy, ox;
                    float v[V];
                    if constexpr (V == 4) {
                        if ((mode & 2) == 0) {                                              // k = 0, 2: along a row of the tile
                            mode_image(mode, T, dy, (mode & 4) ? dx + 3 : dx, oy, ox);
                            const float4 r = *reinterpret_cast<const float4*>(p + oy * T + ox);
                            if (mode & 4) { v[0] = r.w; v[1 % V] = r.z; v[2 % V] = r.y; v[3 % V] = r.x; }
                            else { v[0] = r.x; v[1 % V] = r.y; v[2 % V] = r.z; v[3 % V] = r.w; }
                        } else {
#pragma unroll
                            for (int e = 0; e < V; ++e) {
                                mode_image(mode, T, dy, dx + e, oy, ox);
                                v[e] = p[oy * T + ox];
                            }
                        }
                    } else {
                        mode_image(mode, T, dy, dx, oy, ox);
                        v[0] = p[oy * T + ox];
                    }
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        acc[e] += __fmul_rn(w[e], v[e]);
                        wsum[e] += w[e];
                    }
                }
            }
        }
        const long pi = ((long)c * H + y) * W + x;
        float o[V];
        unsigned char gt[V], q[V];
        if (clean) {
            if constexpr (V == 4) *reinterpret_cast<unsigned*>(gt) = *reinterpret_cast<const unsigned*>(clean + pi);
            else gt[0] = clean[pi];
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            o[e] = acc[e] / wsum[e];
            if (clean) {
                const float d = fminf(fmaxf(o[e], 0.f), 1.f) - __fdiv_rn((float)gt[e], 255.0f);
                sse += d * d;
            }
            q[e] = (unsigned char)fminf(fmaxf(o[e] * 255.0f, 0.f), 255.f);           // image_io.py:383: clip, astype(uint8) truncates
        }
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(packed + pi) = make_float4(o[0], o[1 % V], o[2 % V], o[3 % V]);
            if (u8out) *reinterpret_cast<unsigned*>(u8out + pi) = *reinterpret_cast<const unsigned*>(q);
        } else {
            packed[pi] = o[0];
            if (u8out) u8out[pi] = q[0];
        }
    }
    return sse;
}
__global__ void restore_blend_kernel(const long long* __restrict__ itab, const long long* __restrict__ gtab, const int* __restrict__ ttab,
                                     const float* __restrict__ rest, float* __restrict__ packed, unsigned char* __restrict__ u8out,
                                     float* __restrict__ sse, int i0, int ntiles, int T, int ramp) {
    __shared__ float red[TPB / 64];
    const int im = i0 + blockIdx.y;
    const unsigned char* clean = reinterpret_cast<const unsigned char*>(itab[im * 4 + 0]);
    const int H = (int)itab[im * 4 + 2], W = (int)itab[im * 4 + 3];
    const long long* gt = gtab + (long)im * 8;
    const long off = gt[0];
    const int t0 = (int)gt[1], ny = (int)gt[2], nx = (int)gt[3], stride = (int)gt[4], nmodes = (int)gt[5];
    if (H < 1 || W < 1 || ny < 1 || nx < 1 || stride < 1 || (nmodes != 1 && nmodes != 8)) return;   // a malformed row writes nothing
    float* pk = packed + off;
    unsigned char* u8 = u8out ? u8out + off : nullptr;
    float acc;
    // tile origins are multiples of 4 when the stride and the width are (T % 4 == 0; a padded image starts at 0)
    if ((((long)clean | (long)u8 | off | W | stride) & 3) == 0 && ((long)pk & 15) == 0)
        acc = restore_blend_body<4>(clean, ttab, rest, pk, u8, H, W, t0, ny, nx, stride, nmodes, ntiles, T, ramp);
    else
        acc = restore_blend_body<1>(clean, ttab, rest, pk, u8, H, W, t0, ny, nx, stride, nmodes, ntiles, T, ramp);
    if (!clean) return;
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) atomicAdd(sse + im, acc);
}

// ---- training batch with rain, haze and motion blur synthesised in the launch -------------------------------------------------------
// prm[b] = {code, p1, p2, p3, p4, 0, 0, 0}: code 0 = train_batch_kernel's rule (degraded pointer, or noise, or clean); 1 rain {angle a,
// length L, density16, strength S8}; 2 haze {beta index j, airlight A8}; 3 motion blur {angle a, odd tap count n}.  ray: int8
// [32][32][2] = (dy, dx) of step t along angle a; hazet: uint16 [16][256] transmission * 65535 (fwair/augment.py builds both in f64).
// Every degraded value is integer arithmetic on the SOURCE pixel of the full image, so the two crops of a slot, whatever their modes,
// cut one degraded image that is never stored.  Parameters are clamped to the tables' extent: a malformed record reads nothing outside.
struct SynthSlot {
    int code, a, n, dens, s8;                         // n: taps (blur), length (rain), airlight (haze); a: angle or beta index
};
FW_DEV SynthSlot synth_slot(const int* __restrict__ p) {
    SynthSlot s;
    s.code = p[0];
    s.a = s.code == 2 ? (p[1] & 15) : (p[1] & 31);
    if (s.code == 1) s.n = min(max(p[2], 1), 32);
    else if (s.code == 2) s.n = min(max(p[2], 0), 255);
    else s.n = (min(max(p[2], 1), 25) - 1) | 1;       // odd, 1..25
    s.dens = min(max(p[3], 0), 65536);
    s.s8 = min(max(p[4], 0), 255);
    return s;
}
// steps 0..31 of the slot's angle into LDS (dy[t], dx[t]); every thread of the block calls it
FW_DEV void stage_ray(const signed char* __restrict__ ray, int a, int* sdy, int* sdx) {
    if (threadIdx.x < 32) {
        sdy[threadIdx.x] = ray[(a * 32 + threadIdx.x) * 2 + 0];
        sdx[threadIdx.x] = ray[(a * 32 + threadIdx.x) * 2 + 1];
    }
    __syncthreads();
}
// degraded values d[0..2] (0..255) of source pixel (y, x) of the full image for codes 1..3; g[c] = clean[c][y][x]
FW_DEV void synth_px(const SynthSlot& s, const unsigned char* __restrict__ clean, int H, int W, int y, int x, const int* g, unsigned key,
                     const int* sdy, const int* sdx, const unsigned short* __restrict__ hazet, int* d) {
    if (s.code == 1) {                                                               // rain: the brightest streak that reaches (y, x)
        int m = 0;
        for (int t = 0; t < s.n; ++t) {
            const int qy = y - sdy[t], qx = x - sdx[t];
            if ((unsigned)qy >= (unsigned)H || (unsigned)qx >= (unsigned)W) continue;
            const unsigned h = fw_hash32((unsigned)(qy * W + qx) ^ key);             // one hash per pixel: the same streaks in all channels
            if ((int)(h & 0xFFFFu) < s.dens) m = max(m, (int)(128u + ((h >> 16) & 127u)) * (s.n - t));
        }
        const int add = m * s.s8 / (256 * s.n);
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = min(255, g[c] + add);
    } else if (s.code == 2) {                                                        // haze: depth = a vertical ramp, far at the top
        const int k = H > 1 ? y * 255 / (H - 1) : 0;
        const int T = hazet[s.a * 256 + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (g[c] * T + s.n * (65535 - T) + 32767) / 65535;
    } else {                                                                         // motion blur: n taps along the ray, clamped at the IMAGE border
        int sum[3] = {g[0], g[1], g[2]};
        const long plane = (long)H * W;
        for (int t = 1; t <= (s.n - 1) / 2; ++t) {
            const int dy = sdy[t], dx = sdx[t];
            const long pa = (long)min(max(y + dy, 0), H - 1) * W + min(max(x + dx, 0), W - 1);
            const long pb = (long)min(max(y - dy, 0), H - 1) * W + min(max(x - dx, 0), W - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] += (int)clean[c * plane + pa] + (int)clean[c * plane + pb];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (2 * sum[c] + s.n) / (2 * s.n);
    }
}
// One (slot, view) per blockIdx.y; a thread owns an output pixel in all three channels, so the rain hashes and the blur offsets are
// evaluated once per pixel.  Stores run along ox in every mode.
__global__ void train_batch_synth_kernel(const long long* __restrict__ tab, const int* __restrict__ rnd, const float* __restrict__ sigma,
                                         const int* __restrict__ prm, const signed char* __restrict__ ray,
                                         const unsigned short* __restrict__ hazet, const unsigned* __restrict__ seed, unsigned site,
                                         float* __restrict__ d1, float* __restrict__ d2, float* __restrict__ c1, float* __restrict__ c2, int S) {
    __shared__ int sdy[32], sdx[32];
    const int b = blockIdx.y >> 1, v = blockIdx.y & 1;
    const unsigned char* clean = reinterpret_cast<const unsigned char*>(tab[b * 4 + 0]);
    const unsigned char* degr = reinterpret_cast<const unsigned char*>(tab[b * 4 + 1]);
    const int H = (int)tab[b * 4 + 2], W = (int)tab[b * 4 + 3];
    if (!clean || H < S || W < S) return;                                            // a malformed row reads and writes nothing
    const SynthSlot s = synth_slot(prm + b * 8);
    const bool synth = s.code >= 1 && s.code <= 3;
    if (synth && s.code != 2) stage_ray(ray, s.a, sdy, sdx);                         // uniform in the block
    const int* r = rnd + b * 6 + v * 3;
    const int y0 = (int)((unsigned)r[0] % (unsigned)(H - S + 1)), x0 = (int)((unsigned)r[1] % (unsigned)(W - S + 1));
    const int mode = 1 + (int)((unsigned)r[2] % 7u);
    const unsigned key = fw_site_key(seed[0], site + (unsigned)b);
    const float sg = sigma[b];
    const long plane = (long)H * W;
    float* dout = (v ? d2 : d1) + (long)b * 3 * S * S;
    float* cout = (v ? c2 : c1) + (long)b * 3 * S * S;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < S * S; i += gridDim.x * blockDim.x) {
        const int ox = i % S, oy = i / S;
        int py, px;
        mode_preimage(mode, S, oy, ox, py, px);
        const int y = y0 + py, x = x0 + px;
        const long pi = (long)y * W + x;
        int g[3], d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = clean[c * plane + pi];
        if (synth) synth_px(s, clean, H, W, y, x, g, key, sdy, sdx, hazet, d);
        else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (degr) d[c] = degr[c * plane + pi];
                else if (sg > 0.f) d[c] = (int)noisy_u8((float)g[c], sg, key, c * plane + pi);
                else d[c] = g[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            dout[(long)c * S * S + i] = __fdiv_rn((float)d[c], 255.0f);
            cout[(long)c * S * S + i] = __fdiv_rn((float)g[c], 255.0f);
        }
    }
}
// The degraded image itself (uint8 [3][H][W]) of one sample, by synth_px: for inspection.  Codes 1..3 only.
__global__ void synth_image_kernel(const unsigned char* __restrict__ clean, const int* __restrict__ prm, const signed char* __restrict__ ray,
                                   const unsigned short* __restrict__ hazet, const unsigned* __restrict__ seed, unsigned site,
                                   unsigned char* __restrict__ out, int H, int W) {
    __shared__ int sdy[32], sdx[32];
    const SynthSlot s = synth_slot(prm);
    if (s.code < 1 || s.code > 3) return;
    stage_ray(ray, s.code == 2 ? 0 : s.a, sdy, sdx);
    const unsigned key = fw_site_key(seed[0], site);
    const long plane = (long)H * W;
    for (long i = gtid(); i < plane; i += gstride()) {
        const int x = (int)(i % W), y = (int)(i / W);
        int g[3], d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = clean[c * plane + i];
        synth_px(s, clean, H, W, y, x, g, key, sdy, sdx, hazet, d);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c * plane + i] = (unsigned char)d[c];
    }
}
}  // namespace

#define ST ((hipStream_t)stream)
extern "C" int fw_train_batch(const void* tab, const int* rnd, const float* sigma, const void* seed, int site, float* d1, float* d2, float* c1,
                              float* c2, int B, int S, void* stream) {
    FW_CHECK_ARG(tab && rnd && sigma && seed && d1 && d2 && c1 && c2 && B > 0 && S > 0);
    hipLaunchKernelGGL(train_batch_kernel, dim3(grid_for((long)B * 6 * S * S)), dim3(TPB), 0, ST, (const long long*)tab, rnd, sigma,
                       (const unsigned*)seed, (unsigned)site, d1, d2, c1, c2, B, S);
    FW_LAUNCH_RET();
}
extern "C" int fw_train_batch_synth(const void* tab, const int* rnd, const float* sigma, const int* prm, const void* ray, const void* hazet,
                                    const void* seed, int site, float* d1, float* d2, float* c1, float* c2, int B, int S, void* stream) {
    FW_CHECK_ARG(tab && rnd && sigma && prm && ray && hazet && seed && d1 && d2 && c1 && c2 && B > 0 && B <= 32767 && S > 0 && S <= 4096);
    hipLaunchKernelGGL(train_batch_synth_kernel, dim3((unsigned)((S * S + TPB - 1) / TPB), (unsigned)(2 * B)), dim3(TPB), 0, ST,
                       (const long long*)tab, rnd, sigma, prm, (const signed char*)ray, (const unsigned short*)hazet, (const unsigned*)seed,
                       (unsigned)site, d1, d2, c1, c2, S);
    FW_LAUNCH_RET();
}
extern "C" int fw_synth_image(const void* clean, const int* prm, const void* ray, const void* hazet, const void* seed, int site, void* out,
                              int H, int W, void* stream) {
    FW_CHECK_ARG(clean && prm && ray && hazet && seed && out && H > 0 && W > 0 && (long)H * W < (1L << 31));
    hipLaunchKernelGGL(synth_image_kernel, dim3(grid_for((long)H * W)), dim3(TPB), 0, ST, (const unsigned char*)clean, prm,
                       (const signed char*)ray, (const unsigned short*)hazet, (const unsigned*)seed, (unsigned)site, (unsigned char*)out, H, W);
    FW_LAUNCH_RET();
}
extern "C" int fw_tile_gather(const float* img, const int* ys, const int* xs, float* tiles, int C, int H, int W, int ny, int nx, int T,
                              void* stream) {
    FW_CHECK_ARG(img && ys && xs && tiles && C > 0 && T > 0 && H >= T && W >= T && ny > 0 && nx > 0);
    hipLaunchKernelGGL(tile_gather_kernel, dim3(grid_for((long)ny * nx * C * T * T)), dim3(TPB), 0, ST, img, ys, xs, tiles, C, H, W, ny, nx, T);
    FW_LAUNCH_RET();
}
extern "C" int fw_tile_blend(const float* tiles, const int* ys, const int* xs, float* out, int C, int H, int W, int ny, int nx, int T,
                             void* stream) {
    FW_CHECK_ARG(tiles && ys && xs && out && C > 0 && T > 0 && H >= T && W >= T && ny > 0 && nx > 0);
    hipLaunchKernelGGL(tile_blend_kernel, dim3(grid_for((long)C * H * W)), dim3(TPB), 0, ST, tiles, ys, xs, out, C, H, W, ny, nx, T);
    FW_LAUNCH_RET();
}
extern "C" int fw_ssim7(const float* a, const float* b, float* out, int n, int C, int H, int W, void* stream) {
    FW_CHECK_ARG(a && b && out && n > 0 && C > 0 && H >= 7 && W >= 7);
    const long per = (long)C * (H - 6) * (W - 6);
    long gx = (per + TPB - 1) / TPB;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(ssim7_kernel, dim3((unsigned)gx, (unsigned)n), dim3(TPB), 0, ST, a, b, out, n, C, H, W);
    FW_LAUNCH_RET();
}
extern "C" int fw_eval_gather(const void* itab, const int* ttab, const float* sigma, const void* seed, int site, float* tiles, int N, int T,
                              void* stream) {
    FW_CHECK_ARG(itab && ttab && sigma && seed && tiles && N > 0 && N <= 65535 && T > 0 && T % 4 == 0 && ((uintptr_t)tiles & 15) == 0);
    long gx = ((long)3 * T * T / 4 + TPB - 1) / TPB;
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(eval_gather_kernel, dim3((unsigned)gx, (unsigned)N), dim3(TPB), 0, ST, (const long long*)itab, ttab, sigma,
                       (const unsigned*)seed, (unsigned)site, tiles, T);
    FW_LAUNCH_RET();
}
extern "C" int fw_eval_blend(const void* itab, const void* gtab, const int* ttab, const float* rest, float* packed, void* u8out, float* sse,
                             int i0, int nimg, int ntiles, int T, void* stream) {
    FW_CHECK_ARG(itab && gtab && ttab && rest && packed && sse && i0 >= 0 && nimg > 0 && nimg <= 65535 && ntiles > 0 && T > 0 && T % 4 == 0 &&
                 ((uintptr_t)rest & 15) == 0);
    hipLaunchKernelGGL(eval_blend_kernel, dim3(64, (unsigned)nimg), dim3(TPB), 0, ST, (const long long*)itab, (const long long*)gtab, ttab,
                       rest, packed, (unsigned char*)u8out, sse, i0, ntiles, T);
    FW_LAUNCH_RET();
}
extern "C" int fw_restore_gather(const void* itab, const int* ttab, const float* sigma, const void* seed, int site, float* tiles, int N, int T,
                                 void* stream) {
    FW_CHECK_ARG(itab && ttab && sigma && seed && tiles && N > 0 && N <= 65535 && T > 0 && T % 4 == 0 && ((uintptr_t)tiles & 15) == 0);
    long gx = ((long)3 * T * T / 4 + TPB - 1) / TPB;
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(restore_gather_kernel, dim3((unsigned)gx, (unsigned)N), dim3(TPB), 0, ST, (const long long*)itab, ttab, sigma,
                       (const unsigned*)seed, (unsigned)site, tiles, T);
    FW_LAUNCH_RET();
}
extern "C" int fw_restore_blend(const void* itab, const void* gtab, const int* ttab, const float* rest, float* packed, void* u8out, float* sse,
                                int i0, int nimg, int ntiles, int T, int ramp, void* stream) {
    FW_CHECK_ARG(itab && gtab && ttab && rest && packed && sse && i0 >= 0 && nimg > 0 && nimg <= 65535 && ntiles > 0 && T > 0 && T % 4 == 0 &&
                 ramp >= 1 && (ramp == 1 || ramp <= T / 2) && ((uintptr_t)rest & 15) == 0);
    hipLaunchKernelGGL(restore_blend_kernel, dim3(64, (unsigned)nimg), dim3(TPB), 0, ST, (const long long*)itab, (const long long*)gtab, ttab,
                       rest, packed, (unsigned char*)u8out, sse, i0, ntiles, T, ramp);
    FW_LAUNCH_RET();
}
extern "C" int fw_eval_ssim7(const void* itab, const void* gtab, const float* packed, float* out, int i0, int nimg, void* stream) {
    FW_CHECK_ARG(itab && gtab && packed && out && i0 >= 0 && nimg > 0 && nimg <= 65535);
    hipLaunchKernelGGL(eval_ssim7_kernel, dim3(64, (unsigned)nimg), dim3(TPB), 0, ST, (const long long*)itab, (const long long*)gtab, packed,
                       out, i0);
    FW_LAUNCH_RET();
}
