// Tiled 2-D DFT band decomposition for maps larger than one CU's LDS: square N x N, N a multiple of 64, 192 <= N <= 512
// (K6 at --patch_size 384 / 512; net/utils/frequency_decompose.py:28-118).  fw_heads.hip keeps the kernels for N <= 256.
//
// Every transform is a chain of N^3 real products on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation -- the
// arithmetic class of dft2_decompose_mfma_kernel), run as PASSES over an HBM work buffer.  With W = C - iS (C, S the symmetric
// cos / sin panels of 2 pi u i / N) one pass is ONE kernel,
//     out[p][d] = sum_k in[d][k] . P[k][p]          in, out complex or real, P = W or conj(W), stored TRANSPOSED,
// so the contraction always runs along the contiguous axis of its input and every pass writes 16-byte pieces:
//     row pass       T^t[v][y]   = sum_x x[y][x]     W[x][v]                      real in,  complex out
//     column pass    F[u][v]     = sum_y T^t[v][y]   W[y][u]                      complex,  complex              (the spectrum)
//     band pass      Z^t[c][u]   = sum_v M_b F[u][v] conj(W)[v][c]                mask applied to the fragment as it is loaded
//     output pass    out[r][c]   = Re sum_u Z^t[c][u] conj(W)[u][r] / N^2         complex in, real out
// A workgroup (4 waves, 2 x 2) owns one 64 x 64 output tile of one map and walks K = N in 16-float chunks; a wave's 32 x 32
// quadrant is 2 x 2 MFMA tiles.  Both operands are read as ready-made fragments through L2 (a lane's 16 bytes of a 64-byte
// row chunk): a tile's operands are 64 rows of data and 64 rows of three panels, 20 KB per chunk against 64 MFMAs per wave,
// so the kernels keep NO tile in LDS and the grid is (N/64)^2 tiles per map -- 64 workgroups per map at N = 512.
// The tile walk is generic in N / 64; nothing assumes a power of two.
#include "fw_common.h"

extern "C" int fw_band_residual(const float* img, float* out, int nimg, int N, int nbands, void* stream);

namespace {

// dft_pass_kernel's chunk: DftChunk (fw_common.h) -- the fragments and mac(), the order of MFMAs -- with a loader of its own, which
// multiplies the mask in and takes the three planes as pointers (null: not loaded).  The loader stays here because the kernel's
// schedule follows it: on DftChunk's load_data / load_panels the same kernel needed 4 to 8 more VGPRs and ran slower
// (profiles/r16_dft_tile_ab.json, profiles/r16_dft_tile_meta.txt).
template <bool REAL_IN, bool REAL_OUT, bool MASKED> struct DftFrags : DftChunk<REAL_IN, REAL_OUT, false> {
    // d0 / p0: the wave's first data row / panel row.  P1 carries the imaginary input into the real output, P2 the real input
    // into the imaginary output: (S, -S) for W, (-S, S) for conj(W).
    FW_MEM void load(const float* inr, const float* ini, const float* M, const float* Pc, const float* P1, const float* P2, int N, int d0,
                     int p0, int c) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            this->ar[t] = frag_g(inr, N, d0 + 16 * t, c);
            if (!REAL_IN) this->ai[t] = frag_g(ini, N, d0 + 16 * t, c);
            if (MASKED) {
                const f32x4 m = frag_g(M, N, d0 + 16 * t, c);
                this->ar[t] *= m; this->ai[t] *= m;
            }
            this->pc[t] = frag_g(Pc, N, p0 + 16 * t, c);
            if (P1) this->p1[t] = frag_g(P1, N, p0 + 16 * t, c);
            if (P2) this->p2[t] = frag_g(P2, N, p0 + 16 * t, c);
        }
    }
};

// grid (N/64 panel-row tiles, N/64 data-row tiles, nimg * nbands); 256 threads.  Map z = band * nimg + image.
//   MASKED: every band reads the SAME input map (image z % nimg) through its own mask; otherwise input map z.
//   dc_bits: bit b set = band b is the DC bin alone.  The band pass skips it; the output pass writes dc[image * N * N] * scale.
template <bool REAL_IN, bool REAL_OUT, bool CONJ, bool MASKED>
__global__ __launch_bounds__(256) void dft_pass_kernel(const float* __restrict__ inr, const float* __restrict__ ini, const float* __restrict__ mask,
                                                       const float* __restrict__ panels, float* __restrict__ outr, float* __restrict__ outi,
                                                       const float* __restrict__ dc, int N, int nimg, float scale, unsigned dc_bits) {
    const int w = threadIdx.x >> 6, l = lane_id();
    const int z = blockIdx.z, n = z % nimg, b = z / nimg;
    const size_t NN = (size_t)N * N;
    const int d0 = blockIdx.y * 64 + (w >> 1) * 32, p0 = blockIdx.x * 64 + (w & 1) * 32;
    float* o_r = outr + (size_t)z * NN;
    if (b < 32 && ((dc_bits >> b) & 1u)) {                                  // uniform over the workgroup
        if (REAL_OUT) {
            const float m = dc[(size_t)n * NN] * scale;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    *reinterpret_cast<f32x4*>(o_r + (size_t)(p0 + 16 * nt + (l & 15)) * N + d0 + 16 * mt + ((l >> 4) << 2)) = f32x4{m, m, m, m};
        }
        return;
    }
    const size_t in_off = (size_t)(MASKED ? n : z) * NN;
    const float* xr = inr + in_off;
    const float* xi = REAL_IN ? nullptr : ini + in_off;
    const float* M = MASKED ? mask + (size_t)b * NN : nullptr;
    const float* Pc = panels;
    const float* Ps = panels + NN;
    const float* Pn = panels + 2 * NN;
    const float* P1 = REAL_IN ? nullptr : (CONJ ? Pn : Ps);
    const float* P2 = REAL_OUT ? nullptr : (CONJ ? Ps : Pn);

    f32x4 accr[2][2], acci[2][2];
    zero_acc(accr); zero_acc(acci);
    const int KC = N / 16;
    DftFrags<REAL_IN, REAL_OUT, MASKED> cur, nxt;
    cur.load(xr, xi, M, Pc, P1, P2, N, d0, p0, 0);
    for (int c = 0; c < KC; ++c) {
        if (c + 1 < KC) nxt.load(xr, xi, M, Pc, P1, P2, N, d0, p0, c + 1);  // the next chunk's fragments fly under this chunk's MFMAs
        cur.mac(accr, acci);                                                // consecutive MFMAs go to different accumulators
        cur = nxt;
    }
    // acc element r of lane l is out[m = data row 4 (l >> 4) + r][n = panel row l & 15]: the transpose takes one 16-byte store
    float* o_i = REAL_OUT ? nullptr : outi + (size_t)z * NN;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const size_t o = (size_t)(p0 + 16 * nt + (l & 15)) * N + d0 + 16 * mt + ((l >> 4) << 2);
            *reinterpret_cast<f32x4*>(o_r + o) = accr[mt][nt] * scale;
            if (!REAL_OUT) *reinterpret_cast<f32x4*>(o_i + o) = acci[mt][nt] * scale;
        }
}

// masked spectrum: mode 0 -> (re, im) interleaved, un-shifted (inverse == False);  mode 1 -> |.| in fftshift-ed coordinates ('visual')
__global__ __launch_bounds__(256) void dft_band_spec_kernel(const float* __restrict__ fr, const float* __restrict__ fi, const float* __restrict__ mask,
                                                            float* __restrict__ out, int N, int nimg, int mode) {
    const int n = blockIdx.x, band = blockIdx.y, u = blockIdx.z;
    const size_t NN = (size_t)N * N;
    const float* Fr = fr + n * NN + (size_t)u * N;
    const float* Fi = fi + n * NN + (size_t)u * N;
    const float* M = mask + band * NN + (size_t)u * N;
    float* ob = out + ((size_t)band * nimg + n) * NN * (mode == 0 ? 2 : 1);
    const int us = (u + N / 2) % N;
    for (int v = threadIdx.x; v < N; v += 256) {
        const float m = M[v], a = Fr[v] * m, c = Fi[v] * m;
        if (mode == 0) {
            *reinterpret_cast<float2*>(ob + ((size_t)u * N + v) * 2) = make_float2(a, c);
        } else {
            ob[(size_t)us * N + (v + N / 2) % N] = sqrtf(a * a + c * c);
        }
    }
}

bool dft_tiled_side(int N) { return N >= 192 && N <= 512 && N % 64 == 0; }

}  // namespace

#define ST ((hipStream_t)stream)
#define DFT_PASS(RI, RO, CJ, MK, maps, ...) \
    hipLaunchKernelGGL((dft_pass_kernel<RI, RO, CJ, MK>), dim3(N / 64, N / 64, (unsigned)(maps)), dim3(256), 0, ST, __VA_ARGS__)

// Spectrum of nimg real maps: fr, fi [nimg][N][N] un-shifted (the contract of fw_dft2_fwd).  work: 2 * nimg * N * N floats.
extern "C" int fw_dft2t_fwd(const float* img, const float* panels, float* work, float* fr, float* fi, int nimg, int N, void* stream) {
    FW_CHECK_ARG(img && panels && work && fr && fi && nimg > 0 && nimg <= 65535 && dft_tiled_side(N));
    const size_t per = (size_t)nimg * N * N;
    DFT_PASS(true, false, false, false, nimg, img, nullptr, nullptr, panels, work, work + per, nullptr, N, nimg, 1.0f, 0u);
    DFT_PASS(false, false, false, false, nimg, work, work + per, nullptr, panels, fr, fi, nullptr, N, nimg, 1.0f, 0u);
    FW_LAUNCH_RET();
}
// The contract of fw_dft2_bands.  mode 0: out [nb][nimg][N][N] = Re IDFT2(mask_b . F), work: 2 * nbands * nimg * N * N floats;
// mode 1: (re, im) pairs [nb][nimg][N][N][2];  mode 2: magnitudes, fftshift-ed.  Modes 1 and 2 use neither work nor panels.
extern "C" int fw_dft2t_bands(const float* fr, const float* fi, const float* mask_unshifted, const float* panels, float* work, float* out,
                              int nimg, int N, int nbands, int mode, void* stream) {
    FW_CHECK_ARG(fr && fi && mask_unshifted && out && nimg > 0 && nbands > 0 && (long)nimg * nbands <= 65535 && mode >= 0 && mode <= 2 &&
                 dft_tiled_side(N) && (mode != 0 || (panels && work)));
    if (mode == 0) {
        const int maps = nimg * nbands;
        const size_t per = (size_t)maps * N * N;
        DFT_PASS(false, false, true, true, maps, fr, fi, mask_unshifted, panels, work, work + per, nullptr, N, nimg, 1.0f, 0u);
        DFT_PASS(false, true, true, false, maps, work, work + per, nullptr, panels, out, nullptr, nullptr, N, nimg, 1.0f / ((float)N * (float)N), 0u);
    } else {
        hipLaunchKernelGGL(dft_band_spec_kernel, dim3(nimg, nbands, N), dim3(256), 0, ST, fr, fi, mask_unshifted, out, N, nimg, mode - 1);
    }
    FW_LAUNCH_RET();
}
// The contract of fw_dft2_decompose (a PARTITIONING mask set): out[b] = Re IDFT2(mask_b . DFT2(img)) for b < nbands - 1, a band
// flagged in dc_bits is the image mean (no transform), out[nbands-1] = img - the others.  work: (2 + 2 * nbands) * nimg * N * N floats.
extern "C" int fw_dft2t_decompose(const float* img, const float* mask, const float* panels, float* work, float* out, int nimg, int N,
                                  int nbands, int dc_bits, void* stream) {
    FW_CHECK_ARG(img && mask && panels && work && out && nimg > 0 && nbands >= 2 && nbands <= 31 && (long)nimg * nbands <= 65535 &&
                 dft_tiled_side(N));
    const size_t per = (size_t)nimg * N * N;
    float* Tr = work; float* Ti = work + per; float* Fr = work + 2 * per; float* Fi = work + 3 * per;
    float* Zr = work + 4 * per; float* Zi = Zr + (size_t)(nbands - 1) * per;
    const int maps = nimg * (nbands - 1);
    DFT_PASS(true, false, false, false, nimg, img, nullptr, nullptr, panels, Tr, Ti, nullptr, N, nimg, 1.0f, 0u);
    DFT_PASS(false, false, false, false, nimg, Tr, Ti, nullptr, panels, Fr, Fi, nullptr, N, nimg, 1.0f, 0u);
    DFT_PASS(false, false, true, true, maps, Fr, Fi, mask, panels, Zr, Zi, nullptr, N, nimg, 1.0f, (unsigned)dc_bits);
    DFT_PASS(false, true, true, false, maps, Zr, Zi, nullptr, panels, out, nullptr, Fr, N, nimg, 1.0f / ((float)N * (float)N), (unsigned)dc_bits);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return fw_band_residual(img, out, nimg, N, nbands, stream);
}
