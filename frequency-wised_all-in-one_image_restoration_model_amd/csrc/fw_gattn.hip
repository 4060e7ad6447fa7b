// Global multi-head attention of the ViT encoder plug-in, forward + backward (BASELINE configs[4]: N = 256 tokens at 256x256).
//
// Replaces, per (image, head):  net/encoder_ViT.py:76-98 (`Attention.forward`)
//     dots = q k^T * scale;  attn = softmax(dots);
//     [attn += sum_i lamb[i] * band_i(attn)        the learned band re-weighting of :85-92, frequency_decompose_type != 'none']
//     attn = dropout(attn);  out = attn v
// q | k | v are the three column blocks of the `to_qkv` output ('b n (h d) -> b h n d', head h at column h * 64).
//
// MI355X design.  head_dim is 64 and N = 64 * NT with NT in {1, 4}: one workgroup of 4 waves owns one 64-query tile of one
// (image, head) and sees ALL N keys at once -- the 64 x N score block lives in registers (wave w: queries 16w..16w+15, all keys;
// 4 * NT MFMA tiles), so the softmax is exact (no online rescaling) and costs two shuffles per row.  Every contraction is an MFMA
// product of LDS tiles (fw_common.h): scores are formed TRANSPOSED (S^T = K Q^T: keys along the registers, queries along the
// lanes), so that the C/D layout's 4-consecutive-rows-per-lane is written back to LDS with one 8/16-byte store as the
// k-contiguous operand of the next product, and V / dO / Q / K are read along their token axis with ds_read_b64_tr_b16.
// Dropout masks are counter-based (fw_common.h: fw_keep): the backward pass re-derives them, nothing is stored.
// The band re-weighting at N = 64 (the reference sizes its masks dim_head x dim_head, encoder_ViT.py:56,60; N = 256 with N x N masks:
// the V_* variants and the bands_* passes further down) is a full 64x64
// 2-D DFT on the f32 MFMA (exact f32 products): A' = A + Re F^-1( W . F(A) ), W[u][v] = lamb[band(u, v)], with the cos / sin
// panels read as ready-made fragments from L2; it is self-adjoint (real radial W), so the backward pass runs the same routine on
// the incoming gradient and gets d(lamb) from the two spectra.
// Backward (flash style, deterministic, no atomics on activations): workgroup (image, head, tile t) first acts for QUERY tile t
// (loops over the key tiles: dQ), then for KEY tile t (loops over the query tiles: dK, dV), recomputing P from the saved
// log-sum-exp; with NT = 1 both roles share one pass.
// Any other N = 64 nt up to 1024 (N = 576 at 384x384, 1024 at 512x512): gattn_stream_fwd_kernel walks the key tiles with an online
// softmax, and the backward body runs with a run-time tile count (NT = 0).  The band re-weighting with N x N masks exists there at
// N = 576 and N = 1024 only: 'DC' as a second, unrescaled accumulator of the streaming forward (the affine form of N = 256), <n>_bands
// as LDS-free 64x64-tile DFT passes between a probabilities and an apply kernel (bandsn_pass_kernel; fw_gattn_bands_fwd / bwd serve all three N).
#include "fw_common.h"

namespace {

struct GAttnArgs {
    const char* q; const char* k; const char* v; long ld;      // T; row = token (b * N + n), head h at column h * 64; ld in elements
    char* out; long ldo;                                        // fwd: O [B*N][heads*64]
    float* lse;                                                 // [B][heads][N]
    int B, heads, N;
    float scale;
    const unsigned* seed; unsigned site; unsigned thresh; float inv_keep;      // dropout on the attention map (thresh == 0: off)
    const float* lamb; int nb; int lamb_batch;                  // lamb [nb][lamb_batch (1 | B)][heads]
    const unsigned char* bandidx;                               // [64][64]: band of spectrum bin (u, v), un-shifted coordinates
    const float* panels;                                        // f32 cos [64][64] then sin [64][64] of 2 pi u i / 64
    // backward
    const char* o;                                              // forward output (dvec kernel only)
    const char* dout; long lddo;
    float* dvec;                                                // [B][heads][N] rowsum(dO . O)
    char* dq; char* dk; char* dv; long ldd;
    float* dlamb;                                               // same layout as lamb, accumulated with atomics
    // N = 256 with <n>_bands on the N x N grid: the map leaves the workgroup (f32 [B][heads][N][N])
    float* map;                                                 // fwd: P, then A' = P + filter(P);  bwd: the saved A'
    float* map2;                                                // bwd: G = dropout'(dO V^T), then dA = G + filter(G)
    float* pmap;                                                // bwd: P rebuilt from lse (the spectrum of P gives d lamb)
};

constexpr int NTH = 256;
FW_DEV int wave_id() { return threadIdx.x >> 6; }
FW_DEV void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
FW_DEV float col_sum(float v) { v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64); return v; }
FW_DEV float col_max(float v) { v = fmaxf(v, __shfl_xor(v, 16, 64)); v = fmaxf(v, __shfl_xor(v, 32, 64)); return v; }

template <typename T> struct GG {
    static constexpr int SZ = TT<T>::SZ;
    static constexpr int LDR = 64 * SZ + 16;          // byte stride of a [rows][64] tile of T (16 B pad: conflict-free fragment reads)
    static constexpr int KC = SZ;                     // 64-byte k-chunks over 64 elements
    static constexpr int GR = 4 * SZ;                 // 16-byte granules per row
    static constexpr int TILE = 64 * LDR;
};
constexpr int LDF = 64 * 4 + 16;                      // f32 [64][64] tile of the spectral filter
constexpr int SLOT = 64 * LDF;

// rows x 64 elements, global (row stride ldb bytes) -> LDS tile; whole workgroup
template <typename T, int ROWS> FW_DEV void load_tile(char* tile, const char* g, long ldb) {
    constexpr int GR = GG<T>::GR, LDR = GG<T>::LDR;
#pragma unroll
    for (int i = 0; i < ROWS * GR / NTH; ++i) {
        const int idx = threadIdx.x + i * NTH, r = idx / GR, s = idx % GR;
        *reinterpret_cast<uint4*>(tile + r * LDR + s * 16) = *reinterpret_cast<const uint4*>(g + r * ldb + s * 16);
    }
}
// 16 rows of an LDS tile -> global; ONE wave
template <typename T> FW_DEV void store_rows16(const char* tile, char* g, long ldb) {
    constexpr int GR = GG<T>::GR, LDR = GG<T>::LDR;
    const int l = lane_id();
#pragma unroll
    for (int i = 0; i < 16 * GR / 64; ++i) {
        const int idx = l + i * 64, r = idx / GR, s = idx % GR;
        *reinterpret_cast<uint4*>(g + r * ldb + s * 16) = *reinterpret_cast<const uint4*>(tile + r * LDR + s * 16);
    }
}
FW_DEV uint4 frag_g(const float* P, int row0, int c) {        // A-operand fragment of a global f32 [64][64] panel
    const int l = lane_id();
    return *reinterpret_cast<const uint4*>(P + (row0 + (l & 15)) * 64 + c * 16 + ((l >> 4) << 2));
}
FW_DEV f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// ---- spectral re-weighting on a 64x64 f32 matrix held in strip layout ---------------------------------------------------------
// in[mt][r] = A[16 mt + 4 (l >> 4) + r][16 w + (l & 15)];  out = Re IDFT2( wv . DFT2(A) ) in the same layout;  wv = W at the lane's
// (u = 16 mt + 4 (l >> 4) + r, v = 16 w + (l & 15)); xr / xi receive the (transposed-index) spectrum before weighting.
// arena: 4 slots of SLOT bytes no wave still uses on entry (the entry barrier makes a second call safe); 3 more barriers inside.
FW_DEV void spectral_filter(const f32x4 (&in)[4], f32x4 (&out)[4], const f32x4 (&wv)[4], f32x4 (&xr)[4], f32x4 (&xi)[4], char* arena,
                            const float* Cg, const float* Sg) {
    const int w = wave_id();
    char* As = arena;                 // [kappa][rho], later Yr / Zr
    char* Tr = arena + SLOT;
    char* Ti = arena + 2 * SLOT;
    char* Yi = arena + 3 * SLOT;
    char* Yr = As;
    char* mine = As + 16 * w * LDF;
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) store_acc_T<float>(mine, LDF, 16 * mt, 0, in[mt]);
    wave_fence();
    f32x4 p1[4], p2[4], p3[4], p4[4];
    // G1: T[kappa][v] = sum_rho A[rho][kappa] F[rho][v], F = C - iS;  acc(m = v, n = kappa)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) { p1[mt] = zero4(); p2[mt] = zero4(); }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint4 bf = frag_kc(mine, LDF, 0, c);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            mma_chunk<float>(p1[mt], frag_g(Cg, 16 * mt, c), bf);
            mma_chunk<float>(p2[mt], frag_g(Sg, 16 * mt, c), bf);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        store_acc_T<float>(Tr + 16 * w * LDF, LDF, 16 * mt, 0, p1[mt]);          // Ts[kappa][v], v contiguous
        store_acc_T<float>(Ti + 16 * w * LDF, LDF, 16 * mt, 0, -p2[mt]);
    }
    __syncthreads();
    // G2: X[u][v] = sum_kappa F[u][kappa] T[kappa][v];  acc(m = u, n = v own strip); B operand = Ts read k-major
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) { p1[mt] = zero4(); p2[mt] = zero4(); p3[mt] = zero4(); p4[mt] = zero4(); }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint4 br = frag_km<float>(Tr, LDF, 16 * w, c), bi = frag_km<float>(Ti, LDF, 16 * w, c);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const uint4 cf = frag_g(Cg, 16 * mt, c), sf = frag_g(Sg, 16 * mt, c);
            mma_chunk<float>(p1[mt], cf, br); mma_chunk<float>(p2[mt], sf, bi);
            mma_chunk<float>(p3[mt], cf, bi); mma_chunk<float>(p4[mt], sf, br);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        xr[mt] = p1[mt] + p2[mt];                                               // (C - iS)(Tr + iTi)
        xi[mt] = p3[mt] - p4[mt];
        store_acc_T<float>(Yr + 16 * w * LDF, LDF, 16 * mt, 0, xr[mt] * wv[mt]); // Ys[v][u], u contiguous, rows v = own strip
        store_acc_T<float>(Yi + 16 * w * LDF, LDF, 16 * mt, 0, xi[mt] * wv[mt]);
    }
    wave_fence();
    // G3: Z[kappa][v] = sum_u conj(F)[kappa][u] Y[u][v];  acc(m = kappa, n = v own strip)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) { p1[mt] = zero4(); p2[mt] = zero4(); p3[mt] = zero4(); p4[mt] = zero4(); }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint4 br = frag_kc(Yr + 16 * w * LDF, LDF, 0, c), bi = frag_kc(Yi + 16 * w * LDF, LDF, 0, c);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const uint4 cf = frag_g(Cg, 16 * mt, c), sf = frag_g(Sg, 16 * mt, c);
            mma_chunk<float>(p1[mt], cf, br); mma_chunk<float>(p2[mt], sf, bi);
            mma_chunk<float>(p3[mt], cf, bi); mma_chunk<float>(p4[mt], sf, br);
        }
    }
    wave_fence();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {                                            // (C + iS)(Yr + iYi) -> Zs[v][kappa], kappa contiguous
        store_acc_T<float>(Yr + 16 * w * LDF, LDF, 16 * mt, 0, p1[mt] - p2[mt]);
        store_acc_T<float>(Yi + 16 * w * LDF, LDF, 16 * mt, 0, p3[mt] + p4[mt]);
    }
    __syncthreads();
    // G4: out[rho][kappa] = Re sum_v Z[kappa][v] conj(F)[v][rho] / 4096;  acc(m = rho, n = kappa own strip); B = Zs read k-major
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) { p1[mt] = zero4(); p2[mt] = zero4(); }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint4 br = frag_km<float>(Yr, LDF, 16 * w, c), bi = frag_km<float>(Yi, LDF, 16 * w, c);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            mma_chunk<float>(p1[mt], frag_g(Cg, 16 * mt, c), br);
            mma_chunk<float>(p2[mt], frag_g(Sg, 16 * mt, c), bi);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) out[mt] = (p1[mt] - p2[mt]) * (1.0f / 4096.0f);
}

// W at the lane's 16 spectrum bins
FW_DEV void lamb_weights(const GAttnArgs& a, int b, int h, f32x4 (&wv)[4]) {
    const int l = lane_id(), v = 16 * wave_id() + (l & 15);
    const float* lam = a.lamb + (long)(a.lamb_batch > 1 ? b : 0) * a.heads + h;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = 16 * mt + 4 * (l >> 4) + r;
            wv[mt][r] = lam[(long)a.bandidx[u * 64 + v] * a.lamb_batch * a.heads];
        }
}

// 'DC' with N x N masks at N = 256 (band 0 = the bin (0, 0), band 1 = the rest) needs no transform: every softmax row sums to 1,
// so the mean of the map is exactly 1 / N and  A' = A + lamb0 mean + lamb1 (A - mean) = (1 + lamb1) A + (lamb0 - lamb1) / N.
FW_DEV void dc_coef(const GAttnArgs& a, int b, int h, float& gain, float& offs) {
    const float* lam = a.lamb + (long)(a.lamb_batch > 1 ? b : 0) * a.heads + h;
    const float l0 = lam[0], l1 = lam[(long)a.lamb_batch * a.heads];
    gain = 1.0f + l1;
    offs = (l0 - l1) / (float)a.N;
}

// ================================================================================================================ forward
// Variants at N = 256 (NT = 4) with N x N band masks; the kernels below wrap this body.
//   V_DC: the affine form above.   <n>_bands: the 256x256 map does not fit a workgroup, so the filter runs between two launches:
//   V_PROBS writes the softmax strip P (f32) and lse and stops; V_APPLY reads A' = P + filter(P) back, applies Dropout, and does A'' V.
enum { V_NONE = 0, V_DC = 1, V_PROBS = 2, V_APPLY = 3, V_MAPS = 4 };
template <typename T, int NT, bool LAMB, int VAR>
FW_DEV void gattn_fwd_body(const GAttnArgs& a) {
    constexpr bool DC = VAR == V_DC;
    using G = GG<T>;
    constexpr int SZ = G::SZ, LDR = G::LDR, KC = G::KC, N = 64 * NT, MT = N / 16;
    constexpr int LDP = N * SZ + 16, JC = N * SZ / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;
    char* Ks = Qs + 64 * LDR;
    char* Vs = Ks + N * LDR;
    char* arena = Vs + N * LDR;
    const int w = wave_id(), l = lane_id();
    int item = blockIdx.x;
    const int qt = item % NT; item /= NT;
    const int h = item % a.heads, b = item / a.heads;
    const long ldb = a.ld * SZ;
    if constexpr (VAR != V_APPLY) {
        load_tile<T, 64>(Qs, a.q + ((long)(b * N + qt * 64) * a.ld + h * 64) * SZ, ldb);
        load_tile<T, N>(Ks, a.k + ((long)b * N * a.ld + h * 64) * SZ, ldb);
    }
    if constexpr (VAR != V_PROBS) load_tile<T, N>(Vs, a.v + ((long)b * N * a.ld + h * 64) * SZ, ldb);
    __syncthreads();
    // S^T strip: s[mt][r] = score(query 16 w + (l & 15), key 16 mt + 4 (l >> 4) + r)
    f32x4 s[MT];
    const int iq = qt * 64 + 16 * w + (l & 15);                        // the lane's query
    float* maprow = nullptr;                                           // the lane's 4-key groups of the f32 map
    if constexpr (VAR == V_PROBS || VAR == V_APPLY) maprow = a.map + ((long)(b * a.heads + h) * N + iq) * N + 4 * (l >> 4);
    if constexpr (VAR == V_APPLY) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) s[mt] = *reinterpret_cast<const f32x4*>(maprow + 16 * mt);
    } else {
        uint4 qf[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) qf[c] = frag_kc(Qs, LDR, 16 * w, c);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            s[mt] = zero4();
#pragma unroll
            for (int c = 0; c < KC; ++c) mma_chunk<T>(s[mt], frag_kc(Ks, LDR, 16 * mt, c), qf[c]);
        }
    float mx = -3.0e38f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[mt][r] *= a.scale; mx = fmaxf(mx, s[mt][r]); }
    mx = col_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[mt][r] = __expf(s[mt][r] - mx); sum += s[mt][r]; }
    sum = col_sum(sum);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) s[mt] *= inv;
    if ((l >> 4) == 0) a.lse[(long)(b * a.heads + h) * N + iq] = mx + __logf(sum);
    }
    if constexpr (VAR == V_PROBS) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<f32x4*>(maprow + 16 * mt) = s[mt];
        return;
    }
    if constexpr (LAMB) {
        f32x4 wv[4], fo[4], xr[4], xi[4];
        lamb_weights(a, b, h, wv);
        spectral_filter(s, fo, wv, xr, xi, arena, a.panels, a.panels + 4096);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) s[mt] += fo[mt];
    }
    if constexpr (DC) {
        float gain, offs;
        dc_coef(a, b, h, gain, offs);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) s[mt] = s[mt] * gain + offs;
    }
    if (a.thresh) {
        const unsigned key = fw_site_key(a.seed[0], a.site);
        const unsigned long long base = ((unsigned long long)(b * a.heads + h) * N + iq) * N;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                s[mt][r] = fw_keep(key, base + 16 * mt + 4 * (l >> 4) + r, a.thresh) ? s[mt][r] * a.inv_keep : 0.f;
    }
    __syncthreads();                                                   // every wave is done with K: its space takes the P strips
    char* Ps = Ks + w * 16 * LDP;                                      // [16 queries][N keys] of T
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) store_acc_T<T>(Ps, LDP, 16 * mt, 0, s[mt]);
    wave_fence();
    // O^T[d][i] = sum_j V[j][d] P[i][j]:  A = V read along its token axis, B = the P strip
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = zero4();
#pragma unroll
    for (int c = 0; c < JC; ++c) {
        const uint4 pf = frag_kc(Ps, LDP, 0, c);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) mma_chunk<T>(o[dt], frag_km<T>(Vs, LDR, 16 * dt, c), pf);
    }
    char* Os = Qs + 16 * w * LDR;                                      // rows of Q only this wave ever read
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store_acc_T<T>(Os, LDR, 16 * dt, 0, o[dt]);
    wave_fence();
    store_rows16<T>(Os, a.out + ((long)(b * N + qt * 64 + 16 * w) * a.ldo + h * 64) * SZ, a.ldo * SZ);
}
template <typename T, int NT, bool LAMB>
__global__ __launch_bounds__(NTH) void gattn_fwd_kernel(GAttnArgs a) { gattn_fwd_body<T, NT, LAMB, V_NONE>(a); }
template <typename T>
__global__ __launch_bounds__(NTH) void gattn_dc_fwd_kernel(GAttnArgs a) { gattn_fwd_body<T, 4, false, V_DC>(a); }
template <typename T>
__global__ __launch_bounds__(NTH) void gattn_probs_kernel(GAttnArgs a) { gattn_fwd_body<T, 4, false, V_PROBS>(a); }
template <typename T>
__global__ __launch_bounds__(NTH) void gattn_apply_kernel(GAttnArgs a) { gattn_fwd_body<T, 4, false, V_APPLY>(a); }

// ---- streaming forward: any N = 64 * nt, plain attention + Dropout (no lamb) ---------------------------------------------------
// Same grid and ownership as above (one workgroup per (image, head, 64 queries), a lane owns the query 16 w + (l & 15)), but the
// keys pass by in 64-row tiles and the softmax is the online one: per query a running maximum m and a running sum l of
// e_j = exp(s_j - m); when a tile raises m, l AND the four O^T accumulators take the same factor exp(m_old - m_new) before the
// tile's e_j (exponentiated against m_new only) enter either.  l sums every e_j, dropped or not; Dropout scales the e_j that go
// into P V.  After the last tile O /= l and lse = m + log(l): what the register kernel stores, so the backward pass is shared.
// K / V of tile t + 1 are requested into registers before tile t is computed and written to the other LDS buffer after it (one
// barrier per tile); the last tile, peeled off the loop, requests nothing.
// LDS: Q, 2 K tiles, 2 V tiles, the four waves' P strips = 6 * GG<T>::TILE: 55 296 B in bf16 (two workgroups per CU), 104 448 B in
// f32 (one per CU); O leaves through the Q rows of the own strip.
typedef unsigned __attribute__((ext_vector_type(4))) u32x4;            // native vector: the in-flight tile stays in registers
template <typename T> struct StageRegs { u32x4 k[64 * GG<T>::GR / NTH], v[64 * GG<T>::GR / NTH]; };
template <typename T> FW_DEV void stage_request(StageRegs<T>& s, const char* gk, const char* gv, long ldb) {
    constexpr int GR = GG<T>::GR;
#pragma unroll
    for (int i = 0; i < 64 * GR / NTH; ++i) {
        const int idx = threadIdx.x + i * NTH, r = idx / GR, c = idx % GR;
        s.k[i] = *reinterpret_cast<const u32x4*>(gk + r * ldb + c * 16);
        s.v[i] = *reinterpret_cast<const u32x4*>(gv + r * ldb + c * 16);
    }
}
template <typename T> FW_DEV void stage_write(const StageRegs<T>& s, char* Kt, char* Vt) {
    constexpr int GR = GG<T>::GR, LDR = GG<T>::LDR;
#pragma unroll
    for (int i = 0; i < 64 * GR / NTH; ++i) {
        const int idx = threadIdx.x + i * NTH, r = idx / GR, c = idx % GR;
        *reinterpret_cast<u32x4*>(Kt + r * LDR + c * 16) = s.k[i];
        *reinterpret_cast<u32x4*>(Vt + r * LDR + c * 16) = s.v[i];
    }
}
// one key tile of the online softmax: the lane's (m, l) and O^T accumulators take tile t from the LDS tiles Ks / Vs
// DC ('DC' on the N x N grid at N = 576 / 1024, dc_coef): A' = gain P + offs, and the constant term offs sum_j keep_ij inv_keep v_j
// does not depend on the running maximum, so a second O^T accumulator o2 takes V against the 0 / 1 keep strip Ps2 unrescaled
// (Dropout off: the column sum of V); 0 / 1 is exact in T, inv_keep multiplies in f32 at the end.
template <typename T, bool DC = false>
FW_DEV void stream_tile(const GAttnArgs& a, const char* Ks, const char* Vs, char* Ps, const uint4 (&qf)[GG<T>::KC], unsigned key,
                        unsigned long long base, float& m, float& lsum, f32x4 (&o)[4], char* Ps2 = nullptr, f32x4* o2 = nullptr) {
    constexpr int LDR = GG<T>::LDR, KC = GG<T>::KC;
    // S^T tile: s[mt][r] = score(query 16 w + (l & 15), key 64 t + 16 mt + 4 (l >> 4) + r)
    f32x4 s[4];
    float mx = -3.0e38f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        s[mt] = zero4();
#pragma unroll
        for (int c = 0; c < KC; ++c) mma_chunk<T>(s[mt], frag_kc(Ks, LDR, 16 * mt, c), qf[c]);
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[mt][r] *= a.scale; mx = fmaxf(mx, s[mt][r]); }
    }
    const float mn = fmaxf(m, col_max(mx));
    const float alpha = __expf(m - mn);                                // 0 at the first tile (l = 0, O = 0), 1 when m stays
    m = mn;
    float sum = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[mt][r] = __expf(s[mt][r] - mn); sum += s[mt][r]; }
    lsum = lsum * alpha + col_sum(sum);                                // l and O take the same factor; every e_j enters l
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
    if constexpr (!DC) {
        if (a.thresh) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[mt][r] = fw_keep(key, base + 16 * mt + r, a.thresh) ? s[mt][r] * a.inv_keep : 0.f;
        }
    } else {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            f32x4 kp = f32x4{1.f, 1.f, 1.f, 1.f};
            if (a.thresh) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool keep = fw_keep(key, base + 16 * mt + r, a.thresh);
                    s[mt][r] = keep ? s[mt][r] * a.inv_keep : 0.f;
                    kp[r] = keep ? 1.f : 0.f;
                }
            }
            store_acc_T<T>(Ps2, LDR, 16 * mt, 0, kp);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) store_acc_T<T>(Ps, LDR, 16 * mt, 0, s[mt]);
    wave_fence();
    // O^T[d][i] += sum_j V[j][d] e[i][j]
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        const uint4 pf = frag_kc(Ps, LDR, 0, c);
        if constexpr (!DC) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) mma_chunk<T>(o[dt], frag_km<T>(Vs, LDR, 16 * dt, c), pf);
        } else {
            const uint4 kf = frag_kc(Ps2, LDR, 0, c);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const uint4 vf = frag_km<T>(Vs, LDR, 16 * dt, c);
                mma_chunk<T>(o[dt], vf, pf);
                mma_chunk<T>(o2[dt], vf, kf);
            }
        }
    }
}
template <typename T, bool DC = false>
__global__ __launch_bounds__(NTH) void gattn_stream_fwd_kernel(GAttnArgs a) {
    using G = GG<T>;
    constexpr int SZ = G::SZ, LDR = G::LDR, KC = G::KC, TILE = G::TILE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;
    char* Kb = Qs + TILE;                                              // K tiles 0 / 1
    char* Vb = Kb + 2 * TILE;                                          // V tiles 0 / 1
    char* Ps = Vb + 2 * TILE + wave_id() * 16 * LDR;                   // the wave's [16 queries][64 keys] of T
    char* Ps2 = Ps + TILE;                                             // DC: the wave's keep strip
    const int w = wave_id(), l = lane_id();
    const int N = a.N, nt = N >> 6;
    int item = blockIdx.x;
    const int qt = item % nt; item /= nt;
    const int h = item % a.heads, b = item / a.heads;
    const long ldb = a.ld * SZ;
    const char* gk = a.k + ((long)b * N * a.ld + h * 64) * SZ;
    const char* gv = a.v + ((long)b * N * a.ld + h * 64) * SZ;
    load_tile<T, 64>(Qs, a.q + (((long)b * N + qt * 64) * a.ld + h * 64) * SZ, ldb);
    load_tile<T, 64>(Kb, gk, ldb);
    load_tile<T, 64>(Vb, gv, ldb);
    __syncthreads();
    uint4 qf[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) qf[c] = frag_kc(Qs, LDR, 16 * w, c);
    const int iq = qt * 64 + 16 * w + (l & 15);                        // the lane's query
    // flat index of (b, h, iq, key 4 (l >> 4)) in the [B][heads][N][N] map: what the backward derives (pair_grads)
    const unsigned long long row = (unsigned long long)((long)(b * a.heads + h) * N + iq) * (unsigned long long)N + 4 * (l >> 4);
    const unsigned key = a.thresh ? fw_site_key(a.seed[0], a.site) : 0u;
    float m = -3.0e38f, lsum = 0.f;
    f32x4 o[4], o2[DC ? 4 : 1];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = zero4();
    if constexpr (DC) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o2[dt] = zero4();
    }
    for (int t = 0; t + 1 < nt; ++t) {                                 // every tile but the last: tile t + 1 is in flight under tile t
        StageRegs<T> nx;
        stage_request<T>(nx, gk + (long)(t + 1) * 64 * ldb, gv + (long)(t + 1) * 64 * ldb, ldb);
        stream_tile<T, DC>(a, Kb + (t & 1) * TILE, Vb + (t & 1) * TILE, Ps, qf, key, row + (unsigned long long)t * 64, m, lsum, o, Ps2, o2);
        stage_write<T>(nx, Kb + ((t + 1) & 1) * TILE, Vb + ((t + 1) & 1) * TILE);               // last read before the previous barrier
        __syncthreads();
    }
    {   // the last tile requests nothing
        const int t = nt - 1;
        stream_tile<T, DC>(a, Kb + (t & 1) * TILE, Vb + (t & 1) * TILE, Ps, qf, key, row + (unsigned long long)t * 64, m, lsum, o, Ps2, o2);
    }
    const float inv = 1.0f / lsum;
    if constexpr (DC) {                                                // out = gain O / l + offs inv_keep O2
        float gain, offs;
        dc_coef(a, b, h, gain, offs);
        gain *= inv; offs *= a.inv_keep;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = o[dt] * gain + o2[dt] * offs;
    } else {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= inv;
    }
    if ((l >> 4) == 0) a.lse[(long)(b * a.heads + h) * N + iq] = m + __logf(lsum);
    char* Os = Qs + 16 * w * LDR;                                      // rows of Q only this wave ever read (qf is in registers)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store_acc_T<T>(Os, LDR, 16 * dt, 0, o[dt]);
    wave_fence();
    store_rows16<T>(Os, a.out + (((long)b * N + qt * 64 + 16 * w) * a.ldo + h * 64) * SZ, a.ldo * SZ);
}

// ================================================================================================================ backward
// dvec[b][h][i] = sum_d dO[i][d] O[i][d]
template <typename T>
__global__ void gattn_dvec_kernel(GAttnArgs a) {
    const long n = (long)a.B * a.N * a.heads;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int h = (int)(i % a.heads);
        const long row = i / a.heads;
        const T* o = reinterpret_cast<const T*>(a.o) + row * a.ldo + h * 64;
        const T* d = reinterpret_cast<const T*>(a.dout) + row * a.lddo + h * 64;
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < 64 / TT<T>::E16; ++g) {
            float fo[8], fd[8];
            unpack16<T>(*reinterpret_cast<const uint4*>(o + g * TT<T>::E16), fo);
            unpack16<T>(*reinterpret_cast<const uint4*>(d + g * TT<T>::E16), fd);
#pragma unroll
            for (int e = 0; e < TT<T>::E16; ++e) s += fo[e] * fd[e];
        }
        const int bb = (int)(row / a.N), t = (int)(row % a.N);
        a.dvec[((long)bb * a.heads + h) * a.N + t] = s;
    }
}

// One (query tile, key tile) pair: from the LDS tiles Qs / dOs (queries) and Ks / Vs (keys) to the strips
//   p2[mt][r] = P''^T  (what multiplies V: after re-weighting and dropout)      ds[mt][r] = scale * dS^T
// rows = key 16 mt + 4 (l >> 4) + r of the key tile, column = query 16 w + (l & 15) of the query tile.
// DC (N = 256, dc_coef): p2 = gain P + offs; the constant drops out of the softmax gradient (rowsum(P) = 1), so
// ds = scale gain P (G - rowsum(P G)) with G = dropout'(dO V^T) and rowsum(P G) in dvec (gattn_dc_rows_kernel).
// MAPS (N = 256, <n>_bands): the filter ran between launches; p2 = dropout(A') from the saved map, dP = G + filter(G) from map2
// (Dropout' is already inside G), rowsum(P dP) in dvec (gattn_rowdot_kernel).
template <typename T, int NT, bool LAMB, int VAR = V_NONE>
FW_DEV void pair_grads(const GAttnArgs& a, int b, int h, int qi, int kj, const char* Qs, const char* dOs, const char* Ks, const char* Vs,
                       char* arena, f32x4 (&p2)[4], f32x4 (&ds)[4]) {
    constexpr bool DC = VAR == V_DC, MAPS = VAR == V_MAPS;
    using G = GG<T>;
    constexpr int LDR = G::LDR, KC = G::KC;
    const int N = NT ? 64 * NT : a.N;                                 // NT = 0: the tile count is a run-time value (streaming sizes)
    const int w = wave_id(), l = lane_id();
    const int iq = qi * 64 + 16 * w + (l & 15);
    const long rowid = (long)(b * a.heads + h) * N + iq;
    const float lse = a.lse[rowid];
    f32x4 p[4], dp[4];
    {
        uint4 qf[KC], df[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) { qf[c] = frag_kc(Qs, LDR, 16 * w, c); df[c] = frag_kc(dOs, LDR, 16 * w, c); }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            p[mt] = zero4(); dp[mt] = zero4();
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                mma_chunk<T>(p[mt], frag_kc(Ks, LDR, 16 * mt, c), qf[c]);
                mma_chunk<T>(dp[mt], frag_kc(Vs, LDR, 16 * mt, c), df[c]);
            }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) p[mt][r] = __expf(p[mt][r] * a.scale - lse);
    f32x4 wv[4], xr[4], xi[4];
    if constexpr (LAMB) {
        f32x4 fo[4];
        lamb_weights(a, b, h, wv);
        spectral_filter(p, fo, wv, xr, xi, arena, a.panels, a.panels + 4096);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) p2[mt] = p[mt] + fo[mt];
    } else if constexpr (DC) {
        float gain, offs;
        dc_coef(a, b, h, gain, offs);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) { p2[mt] = p[mt] * gain + offs; p[mt] *= gain; }         // p enters ds only: gain P (G - rowsum(P G))
    } else if constexpr (MAPS) {
        const long off = rowid * N + kj * 64 + 4 * (l >> 4);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) p2[mt] = *reinterpret_cast<const f32x4*>(a.map + off + 16 * mt);
    } else {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) p2[mt] = p[mt];
    }
    if (a.thresh) {
        const unsigned key = fw_site_key(a.seed[0], a.site);
        const unsigned long long base = (unsigned long long)rowid * N + kj * 64;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool keep = fw_keep(key, base + 16 * mt + 4 * (l >> 4) + r, a.thresh);
                p2[mt][r] = keep ? p2[mt][r] * a.inv_keep : 0.f;
                dp[mt][r] = keep ? dp[mt][r] * a.inv_keep : 0.f;
            }
    }
    if constexpr (MAPS) {                                             // replaces the product above (the compiler drops it)
        const long off = rowid * N + kj * 64 + 4 * (l >> 4);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) dp[mt] = *reinterpret_cast<const f32x4*>(a.map2 + off + 16 * mt);
    }
    float dsum;
    if constexpr (LAMB) {
        // dP = dP' + filter(dP') (self-adjoint);  d lamb[band] = sum over the band's bins of Re( X_P conj(X_dP') ) / 4096
        f32x4 fo[4], yr[4], yi[4];
        spectral_filter(dp, fo, wv, yr, yi, arena, a.panels, a.panels + 4096);
        const int v = 16 * w + (l & 15);
        for (int band = 0; band < a.nb; ++band) {
            float acc = 0.f;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (a.bandidx[(16 * mt + 4 * (l >> 4) + r) * 64 + v] == band) acc += xr[mt][r] * yr[mt][r] + xi[mt][r] * yi[mt][r];
            acc = wave_sum(acc);
            if (l == 0) atomicAdd(a.dlamb + ((long)band * a.lamb_batch + (a.lamb_batch > 1 ? b : 0)) * a.heads + h, acc * (1.0f / 4096.0f));
        }
        dsum = 0.f;                                                   // the filter mixes rows: D_i = sum_j P dP has to be formed here
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            dp[mt] += fo[mt];
#pragma unroll
            for (int r = 0; r < 4; ++r) dsum += p[mt][r] * dp[mt][r];
        }
        dsum = col_sum(dsum);
    } else {
        dsum = a.dvec[rowid];
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) ds[mt][r] = p[mt][r] * (dp[mt][r] - dsum) * a.scale;
}

template <typename T, int NT, bool LAMB, int DC>                        // DC: V_NONE | V_DC | V_MAPS, handed to pair_grads
FW_DEV void gattn_bwd_body(const GAttnArgs& a) {
    using G = GG<T>;
    constexpr int SZ = G::SZ, LDR = G::LDR, KC = G::KC, TILE = G::TILE;
    const int nt = NT ? NT : a.N >> 6, N = 64 * nt;                    // NT = 0: run-time tile count, every N = 64 nt without lamb
    static_assert(!LAMB || NT == 1, "the 64x64 transform is defined for N = 64 only");
    static_assert(DC == V_NONE || ((NT == 4 || NT == 0) && !LAMB), "the N x N band grid: N = 256, or a run-time tile count (576 / 1024)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;
    char* dOs = Qs + TILE;
    char* Ks = dOs + TILE;
    char* Vs = Ks + TILE;
    char* arena = Vs + TILE;                                           // LAMB: 4 f32 slots; the P'' / dS strips then live in slots 2 / 1
    char* Ps = LAMB ? arena + 2 * SLOT : Vs + TILE;
    char* dSs = LAMB ? arena + SLOT : Ps + TILE;
    const int w = wave_id();
    int item = blockIdx.x;
    const int t = item % nt; item /= nt;
    const int h = item % a.heads, b = item / a.heads;
    const long ldb = a.ld * SZ, lddob = a.lddo * SZ, lddb = a.ldd * SZ;
    const long col = (long)h * 64 * SZ;
    auto rows = [&](const char* base, long ldbytes, int tile) { return base + (long)(b * N + tile * 64) * ldbytes + col; };
    f32x4 p2[4], ds[4], dq[4], dk[4], dv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { dq[i] = zero4(); dk[i] = zero4(); dv[i] = zero4(); }

    // ---- role Q: queries of tile t against every key tile (NT == 1: the one pair also feeds dK / dV)
    load_tile<T, 64>(Qs, rows(a.q, ldb, t), ldb);
    load_tile<T, 64>(dOs, rows(a.dout, lddob, t), lddob);
    for (int kj = 0; kj < nt; ++kj) {
        load_tile<T, 64>(Ks, rows(a.k, ldb, kj), ldb);
        load_tile<T, 64>(Vs, rows(a.v, ldb, kj), ldb);
        __syncthreads();
        pair_grads<T, NT, LAMB, DC>(a, b, h, t, kj, Qs, dOs, Ks, Vs, arena, p2, ds);
        char* myS = dSs + 16 * w * LDR;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) store_acc_T<T>(myS, LDR, 16 * mt, 0, ds[mt]);             // dSs[i][j], j contiguous
        if constexpr (NT == 1) {
            char* myP = Ps + 16 * w * LDR;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) store_acc_T<T>(myP, LDR, 16 * mt, 0, p2[mt]);
        }
        wave_fence();
        // dQ^T[d][i] += sum_j K[j][d] dS[i][j]
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const uint4 bf = frag_kc(myS, LDR, 0, c);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) mma_chunk<T>(dq[dt], frag_km<T>(Ks, LDR, 16 * dt, c), bf);
        }
        if constexpr (NT == 1) {
            __syncthreads();
            // dV^T[d][j] = sum_i dO[i][d] P''[i][j];  dK^T[d][j] = sum_i Q[i][d] dS[i][j]   (wave w: keys 16 w ..)
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const uint4 pf = frag_km<T>(Ps, LDR, 16 * w, c), sf = frag_km<T>(dSs, LDR, 16 * w, c);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    mma_chunk<T>(dv[dt], frag_km<T>(dOs, LDR, 16 * dt, c), pf);
                    mma_chunk<T>(dk[dt], frag_km<T>(Qs, LDR, 16 * dt, c), sf);
                }
            }
        }
        __syncthreads();
    }
    {   // every wave has left the tiles: stage through the Q / K / V rows of the own strip
        char* st = Qs + 16 * w * LDR;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store_acc_T<T>(st, LDR, 16 * dt, 0, dq[dt]);
        if constexpr (NT == 1) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                store_acc_T<T>(Ks + 16 * w * LDR, LDR, 16 * dt, 0, dk[dt]);
                store_acc_T<T>(Vs + 16 * w * LDR, LDR, 16 * dt, 0, dv[dt]);
            }
        }
        wave_fence();
        store_rows16<T>(st, const_cast<char*>(rows(a.dq, lddb, t)) + (long)16 * w * lddb, lddb);
        if constexpr (NT == 1) {
            store_rows16<T>(Ks + 16 * w * LDR, const_cast<char*>(rows(a.dk, lddb, t)) + (long)16 * w * lddb, lddb);
            store_rows16<T>(Vs + 16 * w * LDR, const_cast<char*>(rows(a.dv, lddb, t)) + (long)16 * w * lddb, lddb);
        }
    }
    if constexpr (NT != 1) {
        // ---- role K: keys of tile t against every query tile
        __syncthreads();
        load_tile<T, 64>(Ks, rows(a.k, ldb, t), ldb);
        load_tile<T, 64>(Vs, rows(a.v, ldb, t), ldb);
        for (int qi = 0; qi < nt; ++qi) {
            load_tile<T, 64>(Qs, rows(a.q, ldb, qi), ldb);
            load_tile<T, 64>(dOs, rows(a.dout, lddob, qi), lddob);
            __syncthreads();
            pair_grads<T, NT, LAMB, DC>(a, b, h, qi, t, Qs, dOs, Ks, Vs, arena, p2, ds);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                store_acc_T<T>(Ps + 16 * w * LDR, LDR, 16 * mt, 0, p2[mt]);
                store_acc_T<T>(dSs + 16 * w * LDR, LDR, 16 * mt, 0, ds[mt]);
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const uint4 pf = frag_km<T>(Ps, LDR, 16 * w, c), sf = frag_km<T>(dSs, LDR, 16 * w, c);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    mma_chunk<T>(dv[dt], frag_km<T>(dOs, LDR, 16 * dt, c), pf);
                    mma_chunk<T>(dk[dt], frag_km<T>(Qs, LDR, 16 * dt, c), sf);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            store_acc_T<T>(Ks + 16 * w * LDR, LDR, 16 * dt, 0, dk[dt]);
            store_acc_T<T>(Vs + 16 * w * LDR, LDR, 16 * dt, 0, dv[dt]);
        }
        wave_fence();
        store_rows16<T>(Ks + 16 * w * LDR, const_cast<char*>(rows(a.dk, lddb, t)) + (long)16 * w * lddb, lddb);
        store_rows16<T>(Vs + 16 * w * LDR, const_cast<char*>(rows(a.dv, lddb, t)) + (long)16 * w * lddb, lddb);
    }
}
template <typename T, int NT, bool LAMB>
__global__ __launch_bounds__(NTH) void gattn_bwd_kernel(GAttnArgs a) { gattn_bwd_body<T, NT, LAMB, V_NONE>(a); }
template <typename T, int NT = 4>                                      // NT = 0: run-time tile count (N = 576 / 1024)
__global__ __launch_bounds__(NTH) void gattn_dc_bwd_kernel(GAttnArgs a) { gattn_bwd_body<T, NT, false, V_DC>(a); }
template <typename T, int NT = 4>
__global__ __launch_bounds__(NTH) void gattn_maps_bwd_kernel(GAttnArgs a) { gattn_bwd_body<T, NT, false, V_MAPS>(a); }

// 'DC' at N = 256, ahead of gattn_dc_bwd_kernel: one workgroup per (image, head, 64-query tile) walks all keys and leaves
//   dvec[i] = sum_j P[i][j] G[i][j],  G = dropout'(dO V^T);     d lamb0 += sum(G) / N;     d lamb1 += sum(G . P) - sum(G) / N
// MAPS (<n>_bands): the same walk writes P -> pmap and G -> map2 (f32) for the filter passes instead of reducing them
// NT = 4: N = 256;  NT = 0: the tile count is a run-time value (N = 576 / 1024)
template <typename T, bool MAPS, int NT = 4>
__global__ __launch_bounds__(NTH) void gattn_dc_rows_kernel(GAttnArgs a) {
    using G = GG<T>;
    constexpr int SZ = G::SZ, LDR = G::LDR, KC = G::KC, TILE = G::TILE;
    const int nt = NT ? NT : a.N >> 6, N = 64 * nt;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;
    char* dOs = Qs + TILE;
    char* Ks = dOs + TILE;
    char* Vs = Ks + TILE;
    const int w = wave_id(), l = lane_id();
    int item = blockIdx.x;
    const int t = item % nt; item /= nt;
    const int h = item % a.heads, b = item / a.heads;
    const long ldb = a.ld * SZ, lddob = a.lddo * SZ;
    const long col = (long)h * 64 * SZ;
    auto rows = [&](const char* base, long ldbytes, int tile) { return base + (long)(b * N + tile * 64) * ldbytes + col; };
    load_tile<T, 64>(Qs, rows(a.q, ldb, t), ldb);
    load_tile<T, 64>(dOs, rows(a.dout, lddob, t), lddob);
    const long rowid = (long)(b * a.heads + h) * N + t * 64 + 16 * w + (l & 15);
    const float lse = a.lse[rowid];
    const unsigned key = a.thresh ? fw_site_key(a.seed[0], a.site) : 0u;
    float spg = 0.f, sg = 0.f;
    for (int kj = 0; kj < nt; ++kj) {
        load_tile<T, 64>(Ks, rows(a.k, ldb, kj), ldb);
        load_tile<T, 64>(Vs, rows(a.v, ldb, kj), ldb);
        __syncthreads();
        uint4 qf[KC], df[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c) { qf[c] = frag_kc(Qs, LDR, 16 * w, c); df[c] = frag_kc(dOs, LDR, 16 * w, c); }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            f32x4 p = zero4(), dp = zero4();
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                mma_chunk<T>(p, frag_kc(Ks, LDR, 16 * mt, c), qf[c]);
                mma_chunk<T>(dp, frag_kc(Vs, LDR, 16 * mt, c), df[c]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float g = dp[r];
                if (a.thresh)
                    g = fw_keep(key, (unsigned long long)rowid * N + kj * 64 + 16 * mt + 4 * (l >> 4) + r, a.thresh) ? g * a.inv_keep : 0.f;
                p[r] = __expf(p[r] * a.scale - lse);
                dp[r] = g;
                spg += p[r] * g;
                sg += g;
            }
            if constexpr (MAPS) {
                const long off = rowid * N + kj * 64 + 16 * mt + 4 * (l >> 4);
                *reinterpret_cast<f32x4*>(a.pmap + off) = p;
                *reinterpret_cast<f32x4*>(a.map2 + off) = dp;
            }
        }
        __syncthreads();
    }
    if constexpr (MAPS) return;
    spg = col_sum(spg); sg = col_sum(sg);                              // every lane of a query now holds its row sums
    const bool own = (l >> 4) == 0;
    if (own) a.dvec[rowid] = spg;
    const float tpg = wave_sum(own ? spg : 0.f), tg = wave_sum(own ? sg : 0.f);
    if (l == 0) {
        float* dl = a.dlamb + (long)(a.lamb_batch > 1 ? b : 0) * a.heads + h;
        atomicAdd(dl, tg * (1.0f / (float)N));
        atomicAdd(dl + (long)a.lamb_batch * a.heads, tpg - tg * (1.0f / (float)N));
    }
}

template <typename T> static size_t fwd_lds(int NT, bool lamb) {
    return (size_t)(64 + 2 * 64 * NT) * GG<T>::LDR + (lamb ? 4 * SLOT : 0);
}
template <typename T> static size_t bwd_lds(bool lamb) { return (size_t)4 * GG<T>::TILE + (lamb ? 4 * SLOT : 2 * GG<T>::TILE); }

template <typename T, int NT, bool LAMB> static void launch_fwd(const GAttnArgs& a, hipStream_t st) {
    const size_t lds = fwd_lds<T>(NT, LAMB);
    FW_SET_LDS_ONCE((gattn_fwd_kernel<T, NT, LAMB>), lds);
    hipLaunchKernelGGL((gattn_fwd_kernel<T, NT, LAMB>), dim3(a.B * a.heads * NT), dim3(NTH), lds, st, a);
}
template <typename T, int NT, bool LAMB> static void launch_bwd(const GAttnArgs& a, hipStream_t st) {
    if (!LAMB) {
        const long n = (long)a.B * a.N * a.heads;
        hipLaunchKernelGGL((gattn_dvec_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    }
    const size_t lds = bwd_lds<T>(LAMB);
    FW_SET_LDS_ONCE((gattn_bwd_kernel<T, NT, LAMB>), lds);
    hipLaunchKernelGGL((gattn_bwd_kernel<T, NT, LAMB>), dim3(a.B * a.heads * NT), dim3(NTH), lds, st, a);
}
// N = 64 nt, 128 <= N <= 1024, N != 256: the streaming forward, and the backward body with a run-time tile count (NT = 0)
template <typename T> static void launch_stream(const GAttnArgs& a, bool bwd, hipStream_t st) {
    const int nt = a.N / 64;
    if (!bwd) {
        const size_t lds = (size_t)6 * GG<T>::TILE;
        FW_SET_LDS_ONCE((gattn_stream_fwd_kernel<T>), lds);
        hipLaunchKernelGGL((gattn_stream_fwd_kernel<T>), dim3(a.B * a.heads * nt), dim3(NTH), lds, st, a);
        return;
    }
    const long n = (long)a.B * a.N * a.heads;
    hipLaunchKernelGGL((gattn_dvec_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    const size_t lds = bwd_lds<T>(false);
    FW_SET_LDS_ONCE((gattn_bwd_kernel<T, 0, false>), lds);
    hipLaunchKernelGGL((gattn_bwd_kernel<T, 0, false>), dim3(a.B * a.heads * nt), dim3(NTH), lds, st, a);
}
// 'DC' at N = 576 / 1024: the streaming forward with the second (constant-term) accumulator; the rows and backward kernels of N = 256
// with a run-time tile count
template <typename T> static void launch_stream_dc(const GAttnArgs& a, bool bwd, hipStream_t st) {
    const int nt = a.N / 64;
    if (!bwd) {
        const size_t lds = (size_t)7 * GG<T>::TILE;
        FW_SET_LDS_ONCE((gattn_stream_fwd_kernel<T, true>), lds);
        hipLaunchKernelGGL((gattn_stream_fwd_kernel<T, true>), dim3(a.B * a.heads * nt), dim3(NTH), lds, st, a);
        return;
    }
    const size_t lds_rows = (size_t)4 * GG<T>::TILE, lds = bwd_lds<T>(false);
    FW_SET_LDS_ONCE((gattn_dc_rows_kernel<T, false, 0>), lds_rows);
    hipLaunchKernelGGL((gattn_dc_rows_kernel<T, false, 0>), dim3(a.B * a.heads * nt), dim3(NTH), lds_rows, st, a);
    FW_SET_LDS_ONCE((gattn_dc_bwd_kernel<T, 0>), lds);
    hipLaunchKernelGGL((gattn_dc_bwd_kernel<T, 0>), dim3(a.B * a.heads * nt), dim3(NTH), lds, st, a);
}
// 'DC' at N = 256: the flash-form kernels with the affine re-weighting, no tables and no scratch
template <typename T> static void launch_dc_fwd(const GAttnArgs& a, hipStream_t st) {
    const size_t lds = fwd_lds<T>(4, false);
    FW_SET_LDS_ONCE((gattn_dc_fwd_kernel<T>), lds);
    hipLaunchKernelGGL((gattn_dc_fwd_kernel<T>), dim3(a.B * a.heads * 4), dim3(NTH), lds, st, a);
}
template <typename T> static void launch_dc_bwd(const GAttnArgs& a, hipStream_t st) {
    const size_t lds_rows = (size_t)4 * GG<T>::TILE, lds = bwd_lds<T>(false);
    FW_SET_LDS_ONCE((gattn_dc_rows_kernel<T, false>), lds_rows);
    hipLaunchKernelGGL((gattn_dc_rows_kernel<T, false>), dim3(a.B * a.heads * 4), dim3(NTH), lds_rows, st, a);
    FW_SET_LDS_ONCE((gattn_dc_bwd_kernel<T>), lds);
    hipLaunchKernelGGL((gattn_dc_bwd_kernel<T>), dim3(a.B * a.heads * 4), dim3(NTH), lds, st, a);
}

// ================================================================================ <n>_bands on the 256x256 map: the filter passes
// map += Re IDFT2( W . DFT2(map) ), W[u][v] = lamb[band(u, v)], batched over maps = B * heads, all products on the f32 MFMA with the
// cos / sin panels ([2][256][256] f32, L2-resident) read as ready-made fragments.  One map is 256 KiB of f32, more than a CU's LDS:
//   row pass  (map, 64 rows i):        T[i][v] = sum_j A[i][j] (C - iS)[j][v]              -> work, stored transposed Tt[v][i]
//   col pass  (map, 32 columns v):     X = (C - iS) T,  Y = W . X,  Z = (C + iS) Y          -> work in place, Zt[v][i]
//                                      (backward: the same strip of the spectrum of P gives d lamb[band] = sum Re(X_P conj X_G) / N^2)
//   out pass  (map, 64 rows i):        map[i][j] += Re sum_v Z[i][v] (C + iS)[v][j] / N^2
// A wave owns a 64 x 64 (row, out) or 64 x 32 (col) block of the result: 4 panel fragments feed 16 / 8 MFMA tiles.
constexpr int LDA = 256 * 4 + 16;                    // byte stride of an LDS tile [rows][256] f32
constexpr int LDZ = 64 * 4 + 16;                     // byte stride of an LDS tile [256][64] f32 (read k-major)
constexpr long PLANE = 65536;                        // floats in one 256x256 plane
FW_DEV uint4 pfrag(const float* P, int row0, int c) {           // fragment of a global f32 [256][256] panel: rows row0.., k-chunk c
    const int l = lane_id();
    return *reinterpret_cast<const uint4*>(P + (row0 + (l & 15)) * 256 + c * 16 + ((l >> 4) << 2));
}
FW_DEV uint4 neg4(const uint4& v) { return make_uint4(v.x ^ 0x80000000u, v.y ^ 0x80000000u, v.z ^ 0x80000000u, v.w ^ 0x80000000u); }

__global__ __launch_bounds__(NTH) void bands_row_kernel(const float* __restrict__ map, float* __restrict__ work, const float* __restrict__ panels) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int w = wave_id(), l = lane_id();
    const int m = blockIdx.x >> 2, i0 = (blockIdx.x & 3) * 64;
    const float* A = map + ((long)m * 256 + i0) * 256;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int idx = threadIdx.x + it * NTH, r = idx >> 6, s = idx & 63;
        *reinterpret_cast<uint4*>(smem + r * LDA + s * 16) = *reinterpret_cast<const uint4*>(A + r * 256 + s * 4);
    }
    __syncthreads();
    const float* Cg = panels;
    const float* Sg = panels + PLANE;
    const int v0 = 64 * w;
    f32x4 tr[4][4], ti[4][4];
    zero_acc(tr); zero_acc(ti);
    for (int c = 0; c < 16; ++c) {                                     // acc(m = i, n = v) = sum_j A[i][j] panel[v][j]
        uint4 af[4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) af[mi] = frag_kc(smem, LDA, 16 * mi, c);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const uint4 cf = pfrag(Cg, v0 + 16 * ni, c), sf = pfrag(Sg, v0 + 16 * ni, c);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) { mma_chunk<float>(tr[mi][ni], af[mi], cf); mma_chunk<float>(ti[mi][ni], af[mi], sf); }
        }
    }
    float* Tr = work + (long)m * 2 * PLANE;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const long o = (long)(v0 + 16 * ni + (l & 15)) * 256 + i0 + 16 * mi + 4 * (l >> 4);
            *reinterpret_cast<f32x4*>(Tr + o) = tr[mi][ni];
            *reinterpret_cast<f32x4*>(Tr + PLANE + o) = -ti[mi][ni];
        }
}

// (xr + i xi)[u][v] = sum_k (C -/+ iS)[u][k] (R + iI)[k][v] for u = u0 .. u0 + 63 and the strip's 32 v; Rs / Is: LDS [32 v][256 k]
template <bool CONJ>
FW_DEV void col_dft(const char* Rs, const char* Is, const float* Cg, const float* Sg, int u0, f32x4 (&xr)[4][2], f32x4 (&xi)[4][2]) {
    zero_acc(xr); zero_acc(xi);
    for (int c = 0; c < 16; ++c) {
        uint4 br[2], bi[2];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) { br[ni] = frag_kc(Rs, LDA, 16 * ni, c); bi[ni] = frag_kc(Is, LDA, 16 * ni, c); }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const uint4 cf = pfrag(Cg, u0 + 16 * mi, c), sf = pfrag(Sg, u0 + 16 * mi, c), nsf = neg4(sf);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                mma_chunk<float>(xr[mi][ni], cf, br[ni]); mma_chunk<float>(xr[mi][ni], CONJ ? nsf : sf, bi[ni]);
                mma_chunk<float>(xi[mi][ni], cf, bi[ni]); mma_chunk<float>(xi[mi][ni], CONJ ? sf : nsf, br[ni]);
            }
        }
    }
}

template <bool DL>
__global__ __launch_bounds__(NTH) void bands_col_kernel(float* __restrict__ work, const float* __restrict__ pwork, const float* __restrict__ panels,
                                                        const unsigned char* __restrict__ bandidx, const float* __restrict__ lamb,
                                                        float* __restrict__ dlamb, int nb, int lb, int heads) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float lw[16];
    __shared__ float red[4][16];
    char* Trs = smem;
    char* Tis = Trs + 32 * LDA;
    char* Prs = Tis + 32 * LDA;                                        // DL only
    char* Pis = Prs + 32 * LDA;
    const int w = wave_id(), l = lane_id();
    const int m = blockIdx.x >> 3, v0 = (blockIdx.x & 7) * 32;
    const int h = m % heads, bsel = lb > 1 ? m / heads : 0;
    if (threadIdx.x < nb) lw[threadIdx.x] = lamb[((long)threadIdx.x * lb + bsel) * heads + h];
    float* Tg = work + (long)m * 2 * PLANE + (long)v0 * 256;           // rows v0 .. v0 + 31 of Tt (re), + PLANE: im
    const float* Pg = DL ? pwork + (long)m * 2 * PLANE + (long)v0 * 256 : nullptr;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int idx = threadIdx.x + it * NTH, r = idx >> 6, s = idx & 63;
        *reinterpret_cast<uint4*>(Trs + r * LDA + s * 16) = *reinterpret_cast<const uint4*>(Tg + r * 256 + s * 4);
        *reinterpret_cast<uint4*>(Tis + r * LDA + s * 16) = *reinterpret_cast<const uint4*>(Tg + PLANE + r * 256 + s * 4);
        if constexpr (DL) {
            *reinterpret_cast<uint4*>(Prs + r * LDA + s * 16) = *reinterpret_cast<const uint4*>(Pg + r * 256 + s * 4);
            *reinterpret_cast<uint4*>(Pis + r * LDA + s * 16) = *reinterpret_cast<const uint4*>(Pg + PLANE + r * 256 + s * 4);
        }
    }
    __syncthreads();
    const float* Cg = panels;
    const float* Sg = panels + PLANE;
    const int u0 = 64 * w;
    f32x4 xr[4][2], xi[4][2];
    col_dft<false>(Trs, Tis, Cg, Sg, u0, xr, xi);
    unsigned idx4[4][2];                                               // bands of the lane's bins (u .. u + 3, v); the index is symmetric
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
            idx4[mi][ni] = *reinterpret_cast<const unsigned*>(bandidx + (v0 + 16 * ni + (l & 15)) * 256 + u0 + 16 * mi + 4 * (l >> 4));
    if constexpr (DL) {
        f32x4 pr[4][2], pi[4][2];
        col_dft<false>(Prs, Pis, Cg, Sg, u0, pr, pi);
        for (int band = 0; band < nb; ++band) {
            float acc = 0.f;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (((idx4[mi][ni] >> (8 * r)) & 255u) == (unsigned)band) acc += pr[mi][ni][r] * xr[mi][ni][r] + pi[mi][ni][r] * xi[mi][ni][r];
            acc = wave_sum(acc);
            if (l == 0) red[w][band] = acc;
        }
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float wgt = lw[(idx4[mi][ni] >> (8 * r)) & 255u];
                xr[mi][ni][r] *= wgt; xi[mi][ni][r] *= wgt;
            }
    __syncthreads();                                                   // every wave has read T: its space takes Yt[v][u]
    if constexpr (DL) {
        if (threadIdx.x < nb) {
            const int band = threadIdx.x;
            atomicAdd(dlamb + ((long)band * lb + bsel) * heads + h, (red[0][band] + red[1][band] + red[2][band] + red[3][band]) * (1.0f / 65536.0f));
        }
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            store_acc_T<float>(Trs, LDA, u0 + 16 * mi, 16 * ni, xr[mi][ni]);
            store_acc_T<float>(Tis, LDA, u0 + 16 * mi, 16 * ni, xi[mi][ni]);
        }
    __syncthreads();
    col_dft<true>(Trs, Tis, Cg, Sg, u0, xr, xi);                       // rows i = u0 .. u0 + 63 of Z
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const long o = (long)(16 * ni + (l & 15)) * 256 + u0 + 16 * mi + 4 * (l >> 4);
            *reinterpret_cast<f32x4*>(Tg + o) = xr[mi][ni];
            *reinterpret_cast<f32x4*>(Tg + PLANE + o) = xi[mi][ni];
        }
}

__global__ __launch_bounds__(NTH) void bands_out_kernel(float* __restrict__ map, const float* __restrict__ work, const float* __restrict__ panels) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Zrs = smem;
    char* Zis = smem + 256 * LDZ;
    const int w = wave_id(), l = lane_id();
    const int m = blockIdx.x >> 2, i0 = (blockIdx.x & 3) * 64;
    const float* Zg = work + (long)m * 2 * PLANE + i0;                 // Zt[v][i0 ..]
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int idx = threadIdx.x + it * NTH, r = idx >> 4, s = idx & 15;
        *reinterpret_cast<uint4*>(Zrs + r * LDZ + s * 16) = *reinterpret_cast<const uint4*>(Zg + r * 256 + s * 4);
        *reinterpret_cast<uint4*>(Zis + r * LDZ + s * 16) = *reinterpret_cast<const uint4*>(Zg + PLANE + r * 256 + s * 4);
    }
    __syncthreads();
    const float* Cg = panels;
    const float* Sg = panels + PLANE;
    const int j0 = 64 * w;
    f32x4 o[4][4];
    zero_acc(o);
    for (int c = 0; c < 16; ++c) {                                     // acc(m = j, n = i) = sum_v C[j][v] Zr[i][v] - S[j][v] Zi[i][v]
        uint4 br[4], bi[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) { br[ni] = frag_km<float>(Zrs, LDZ, 16 * ni, c); bi[ni] = frag_km<float>(Zis, LDZ, 16 * ni, c); }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const uint4 cf = pfrag(Cg, j0 + 16 * mi, c), nsf = neg4(pfrag(Sg, j0 + 16 * mi, c));
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) { mma_chunk<float>(o[mi][ni], cf, br[ni]); mma_chunk<float>(o[mi][ni], nsf, bi[ni]); }
        }
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            f32x4* p = reinterpret_cast<f32x4*>(map + ((long)m * 256 + i0 + 16 * ni + (l & 15)) * 256 + j0 + 16 * mi + 4 * (l >> 4));
            *p = *p + o[mi][ni] * (1.0f / 65536.0f);
        }
}

// dvec[row] = sum_j P[row][j] dA[row][j]; one wave per row of 256.  Not gattn_rowdotn_kernel with N = 256: the compiler contracts this
// one expression to an FMA chain and the loop body there to packed multiplies and adds, so the two round differently and each
// size keeps the kernel its pinned bytes came from (tests/test_spec_bits_gpu.py, group gattn_bands).
__global__ __launch_bounds__(NTH) void gattn_rowdot_kernel(const float* __restrict__ P, const float* __restrict__ dA, float* __restrict__ dvec) {
    const long row = (long)blockIdx.x * 4 + wave_id();
    const int l = lane_id();
    const f32x4 p = *reinterpret_cast<const f32x4*>(P + row * 256 + 4 * l), g = *reinterpret_cast<const f32x4*>(dA + row * 256 + 4 * l);
    const float s = wave_sum(p[0] * g[0] + p[1] * g[1] + p[2] * g[2] + p[3] * g[3]);
    if (l == 0) dvec[row] = s;
}

constexpr size_t ROW_LDS = 64 * LDA, COL_LDS = 64 * LDA, OUT_LDS = 2 * 256 * LDZ;
// map += filter(map) over `maps` maps; backward (dlamb != nullptr): also d lamb against the half transform of pmap in pwork
static void launch_filter(float* map, float* work, const float* pmap, float* pwork, const GAttnArgs& a, hipStream_t st) {
    const int maps = a.B * a.heads;
    const bool dl = a.dlamb != nullptr && pmap != nullptr;
    FW_SET_LDS_ONCE(bands_row_kernel, ROW_LDS);
    if (dl) hipLaunchKernelGGL(bands_row_kernel, dim3(maps * 4), dim3(NTH), ROW_LDS, st, pmap, pwork, a.panels);
    hipLaunchKernelGGL(bands_row_kernel, dim3(maps * 4), dim3(NTH), ROW_LDS, st, (const float*)map, work, a.panels);
    if (dl) {
        FW_SET_LDS_ONCE((bands_col_kernel<true>), 2 * COL_LDS);
        hipLaunchKernelGGL((bands_col_kernel<true>), dim3(maps * 8), dim3(NTH), 2 * COL_LDS, st, work, (const float*)pwork, a.panels, a.bandidx, a.lamb,
                           a.dlamb, a.nb, a.lamb_batch, a.heads);
    } else {
        FW_SET_LDS_ONCE((bands_col_kernel<false>), COL_LDS);
        hipLaunchKernelGGL((bands_col_kernel<false>), dim3(maps * 8), dim3(NTH), COL_LDS, st, work, (const float*)nullptr, a.panels, a.bandidx, a.lamb,
                           (float*)nullptr, a.nb, a.lamb_batch, a.heads);
    }
    FW_SET_LDS_ONCE(bands_out_kernel, OUT_LDS);
    hipLaunchKernelGGL(bands_out_kernel, dim3(maps * 4), dim3(NTH), OUT_LDS, st, map, (const float*)work, a.panels);
}
template <typename T> static int bands_fwd(const GAttnArgs& a, float* work, hipStream_t st) {
    const size_t lds = fwd_lds<T>(4, false);
    FW_SET_LDS_ONCE((gattn_probs_kernel<T>), lds);
    hipLaunchKernelGGL((gattn_probs_kernel<T>), dim3(a.B * a.heads * 4), dim3(NTH), lds, st, a);
    launch_filter(a.map, work, nullptr, nullptr, a, st);
    FW_SET_LDS_ONCE((gattn_apply_kernel<T>), lds);
    hipLaunchKernelGGL((gattn_apply_kernel<T>), dim3(a.B * a.heads * 4), dim3(NTH), lds, st, a);
    FW_LAUNCH_RET();
}
template <typename T> static int bands_bwd(const GAttnArgs& a, float* work, hipStream_t st) {
    const int maps = a.B * a.heads;
    const size_t lds_rows = (size_t)4 * GG<T>::TILE, lds = bwd_lds<T>(false);
    FW_SET_LDS_ONCE((gattn_dc_rows_kernel<T, true>), lds_rows);
    hipLaunchKernelGGL((gattn_dc_rows_kernel<T, true>), dim3(maps * 4), dim3(NTH), lds_rows, st, a);
    launch_filter(a.map2, work, a.pmap, work + (long)maps * 2 * PLANE, a, st);
    hipLaunchKernelGGL(gattn_rowdot_kernel, dim3(maps * 64), dim3(NTH), 0, st, (const float*)a.pmap, (const float*)a.map2, a.dvec);
    FW_SET_LDS_ONCE((gattn_maps_bwd_kernel<T>), lds);
    hipLaunchKernelGGL((gattn_maps_bwd_kernel<T>), dim3(maps * 4), dim3(NTH), lds, st, a);
    FW_LAUNCH_RET();
}
// ================================================================= <n>_bands on the 576x576 / 1024x1024 map (384x384 / 512x512 inputs)
// The same statement as at N = 256, map += Re IDFT2( W . DFT2(map) ), but a 64 x N f32 strip (256 KB at N = 1024) no longer fits a
// CU's LDS, so the filter is the LDS-free tile walk of csrc/fw_dft.hip: one pass is one kernel
//     out[p][d] = sum_k in[d][k] P[k][p],     P = C - iS or its conjugate (symmetric panels: rows p are read k-contiguous),
// a workgroup (4 waves, 2 x 2) owns one 64 x 64 output tile of one map, both operands are read as ready-made fragments through L2,
// every product runs on v_mfma_f32_16x16x4_f32, and the result is stored transposed with 16-byte stores:
//     row pass      T^t[v][i] = sum_j A[i][j]   W[j][v]                  real in
//     column pass   X[u][v]   = sum_i T^t[v][i] W[i][u];  Y = lamb[band(u, v)] X on the way out
//                   (backward: the spectrum of P, taken by the same two passes first, gives d lamb[band] = sum Re(X_P conj X_G) / N^2)
//     inverse pass  Z^t[c][u] = sum_v Y[u][v]   conj(W)[v][c]
//     output pass   map[r][c] += Re sum_u Z^t[c][u] conj(W)[u][r] / N^2
// The four partial sums (re C, im S, im C, re S) keep their own accumulators and meet at the end with the signs of W or conj(W), so
// the cos | sin panels of the N = 256 passes serve unchanged.  The tile walk is generic in N / 64.
// This is NOT DftChunk::mac (fw_common.h), on purpose: on DftChunk -- two accumulator sets, a third -sin plane, five fragments per
// tile and chunk where this form loads four -- the complex passes ran 6 to 9 % slower (profiles/r17_gattn_bands_ab.json).
// The fragment loader and the MFMA are fw_common.h's (::frag_g: the frag_g of this file reads the 64x64 panels of the N = 64 filter).
struct BnFrags { f32x4 ar[2], ai[2], pc[2], ps[2]; };
template <bool REAL_IN>
FW_DEV void bn_load(BnFrags& f, const float* xr, const float* xi, const float* Pc, const float* Ps, int N, int d0, int p0, int c) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        f.ar[t] = ::frag_g(xr, N, d0 + 16 * t, c);
        if (!REAL_IN) f.ai[t] = ::frag_g(xi, N, d0 + 16 * t, c);
        f.pc[t] = ::frag_g(Pc, N, p0 + 16 * t, c);
        f.ps[t] = ::frag_g(Ps, N, p0 + 16 * t, c);
    }
}
enum { E_PLAIN = 0, E_WEIGHT = 1, E_WEIGHT_DL = 2 };
// grid (N/64 panel-row tiles, N/64 data-row tiles, maps); 256 threads.  REAL_OUT adds scale * Re(.) to outr (the map) in place.
// EPI: E_WEIGHT multiplies the result by lamb[band(p, d)]; E_WEIGHT_DL first reduces d lamb against the spectrum (pr, pi) of P.
template <bool REAL_IN, bool REAL_OUT, bool CONJ, int EPI>
__global__ __launch_bounds__(NTH) void bandsn_pass_kernel(const float* __restrict__ inr, const float* __restrict__ ini, const float* __restrict__ panels,
                                                          float* __restrict__ outr, float* __restrict__ outi, int N, float scale,
                                                          const unsigned char* __restrict__ bandidx, const float* __restrict__ lamb,
                                                          const float* __restrict__ pr, const float* __restrict__ pi, float* __restrict__ dlamb,
                                                          int nb, int lb, int heads) {
    __shared__ float lw[16];
    __shared__ float red[4][16];
    const int w = wave_id(), l = lane_id();
    const int z = blockIdx.z;
    const size_t NN = (size_t)N * N;
    const int d0 = blockIdx.y * 64 + (w >> 1) * 32, p0 = blockIdx.x * 64 + (w & 1) * 32;
    const int h = z % heads, bsel = lb > 1 ? z / heads : 0;
    if constexpr (EPI != E_PLAIN) {
        if (threadIdx.x < nb) lw[threadIdx.x] = lamb[((long)threadIdx.x * lb + bsel) * heads + h];
        __syncthreads();
    }
    const float* xr = inr + (size_t)z * NN;
    const float* xi = REAL_IN ? nullptr : ini + (size_t)z * NN;
    const float* Pc = panels;
    const float* Ps = panels + NN;
    f32x4 rc[2][2], rs[2][2], ic[2][2], is[2][2];                            // sum ar C, sum ai S, sum ai C, sum ar S
    zero_acc(rc); zero_acc(rs); zero_acc(ic); zero_acc(is);
    const int KC = N / 16;
    BnFrags cur, nxt;
    bn_load<REAL_IN>(cur, xr, xi, Pc, Ps, N, d0, p0, 0);
    for (int c = 0; c < KC; ++c) {
        if (c + 1 < KC) bn_load<REAL_IN>(nxt, xr, xi, Pc, Ps, N, d0, p0, c + 1);   // the next chunk's fragments fly under this chunk's MFMAs
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    FW_MFMA_F32(rc[mt][nt], cur.ar[mt][s], cur.pc[nt][s]);
                    if (!REAL_OUT) FW_MFMA_F32(is[mt][nt], cur.ar[mt][s], cur.ps[nt][s]);
                    if (!REAL_IN) {
                        FW_MFMA_F32(rs[mt][nt], cur.ai[mt][s], cur.ps[nt][s]);
                        if (!REAL_OUT) FW_MFMA_F32(ic[mt][nt], cur.ai[mt][s], cur.pc[nt][s]);
                    }
                }
        cur = nxt;
    }
    // (ar + i ai)(C -/+ iS): re = rc +/- rs, im = ic -/+ is.  acc element r of lane l is out[p = panel row l & 15][d = data row 4 (l >> 4) + r]
    float bacc[16];
    if constexpr (EPI == E_WEIGHT_DL) {
#pragma unroll
        for (int i = 0; i < 16; ++i) bacc[i] = 0.f;
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const size_t o = (size_t)(p0 + 16 * nt + (l & 15)) * N + d0 + 16 * mt + ((l >> 4) << 2);
            f32x4 re = CONJ ? rc[mt][nt] - rs[mt][nt] : rc[mt][nt] + rs[mt][nt];
            if constexpr (REAL_OUT) {
                f32x4* dst = reinterpret_cast<f32x4*>(outr + (size_t)z * NN + o);
                *dst = *dst + re * scale;
            } else {
                f32x4 im = CONJ ? ic[mt][nt] + is[mt][nt] : ic[mt][nt] - is[mt][nt];
                if constexpr (EPI != E_PLAIN) {
                    const unsigned idx4 = *reinterpret_cast<const unsigned*>(bandidx + o);   // bands of (p, d .. d + 3)
                    if constexpr (EPI == E_WEIGHT_DL) {
                        const f32x4 qr = *reinterpret_cast<const f32x4*>(pr + (size_t)z * NN + o);
                        const f32x4 qi = *reinterpret_cast<const f32x4*>(pi + (size_t)z * NN + o);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const unsigned band = (idx4 >> (8 * r)) & 255u;
                            const float v = qr[r] * re[r] + qi[r] * im[r];
#pragma unroll
                            for (int i = 0; i < 16; ++i) bacc[i] += band == (unsigned)i ? v : 0.f;
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float wgt = lw[(idx4 >> (8 * r)) & 15u];
                        re[r] *= wgt; im[r] *= wgt;
                    }
                }
                *reinterpret_cast<f32x4*>(outr + (size_t)z * NN + o) = re * scale;
                *reinterpret_cast<f32x4*>(outi + (size_t)z * NN + o) = im * scale;
            }
        }
    if constexpr (EPI == E_WEIGHT_DL) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float t = wave_sum(bacc[i]);
            if (l == 0) red[w][i] = t;
        }
        __syncthreads();
        if (threadIdx.x < nb) {                                              // one atomic per workgroup and band
            const int band = threadIdx.x;
            atomicAdd(dlamb + ((long)band * lb + bsel) * heads + h,
                      (red[0][band] + red[1][band] + red[2][band] + red[3][band]) / ((float)N * (float)N));
        }
    }
}

// lse and P = exp(s scale - lse) (f32, -> map) of one (image, head, 64-query tile): the key tiles pass by twice, first under the
// online maximum / sum of the streaming forward, then against the finished lse -- the expression the backward pass rebuilds P with.
template <typename T>
__global__ __launch_bounds__(NTH) void gattn_probsn_kernel(GAttnArgs a) {
    using G = GG<T>;
    constexpr int SZ = G::SZ, LDR = G::LDR, KC = G::KC, TILE = G::TILE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;
    char* Ks = Qs + TILE;
    const int w = wave_id(), l = lane_id();
    const int N = a.N, nt = N >> 6;
    int item = blockIdx.x;
    const int qt = item % nt; item /= nt;
    const int h = item % a.heads, b = item / a.heads;
    const long ldb = a.ld * SZ;
    const char* gk = a.k + ((long)b * N * a.ld + h * 64) * SZ;
    load_tile<T, 64>(Qs, a.q + (((long)b * N + qt * 64) * a.ld + h * 64) * SZ, ldb);
    const int iq = qt * 64 + 16 * w + (l & 15);                        // the lane's query
    const long rowid = (long)(b * a.heads + h) * N + iq;
    float m = -3.0e38f, lsum = 0.f, lse = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        for (int t = 0; t < nt; ++t) {
            load_tile<T, 64>(Ks, gk + (long)t * 64 * ldb, ldb);
            __syncthreads();
            uint4 qf[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) qf[c] = frag_kc(Qs, LDR, 16 * w, c);
            // S^T tile: s[mt][r] = score(query 16 w + (l & 15), key 64 t + 16 mt + 4 (l >> 4) + r)
            f32x4 s[4];
            float mx = -3.0e38f;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                s[mt] = zero4();
#pragma unroll
                for (int c = 0; c < KC; ++c) mma_chunk<T>(s[mt], frag_kc(Ks, LDR, 16 * mt, c), qf[c]);
#pragma unroll
                for (int r = 0; r < 4; ++r) { s[mt][r] *= a.scale; mx = fmaxf(mx, s[mt][r]); }
            }
            if (pass == 0) {
                const float mn = fmaxf(m, col_max(mx));
                float sum = 0.f;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sum += __expf(s[mt][r] - mn);
                lsum = lsum * __expf(m - mn) + col_sum(sum);
                m = mn;
            } else {
                float* dst = a.map + rowid * N + t * 64 + 4 * (l >> 4);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[mt][r] = __expf(s[mt][r] - lse);
                    *reinterpret_cast<f32x4*>(dst + 16 * mt) = s[mt];
                }
            }
            __syncthreads();
        }
        if (pass == 0) {
            lse = m + __logf(lsum);
            if ((l >> 4) == 0) a.lse[rowid] = lse;
        }
    }
}

// A' (map, after the filter) -> Dropout with the counter index (b, h, i, j) the backward derives -> O = A'' V, key tile by key tile
template <typename T>
__global__ __launch_bounds__(NTH) void gattn_applyn_kernel(GAttnArgs a) {
    using G = GG<T>;
    constexpr int SZ = G::SZ, LDR = G::LDR, KC = G::KC, TILE = G::TILE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Os = smem + wave_id() * 16 * LDR;                            // the wave's 16 output rows
    char* Vs = smem + TILE;
    char* Ps = smem + 2 * TILE + wave_id() * 16 * LDR;                 // the wave's [16 queries][64 keys] of T
    const int w = wave_id(), l = lane_id();
    const int N = a.N, nt = N >> 6;
    int item = blockIdx.x;
    const int qt = item % nt; item /= nt;
    const int h = item % a.heads, b = item / a.heads;
    const long ldb = a.ld * SZ;
    const char* gv = a.v + ((long)b * N * a.ld + h * 64) * SZ;
    const int iq = qt * 64 + 16 * w + (l & 15);
    const long rowid = (long)(b * a.heads + h) * N + iq;
    const unsigned key = a.thresh ? fw_site_key(a.seed[0], a.site) : 0u;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = zero4();
    for (int t = 0; t < nt; ++t) {
        load_tile<T, 64>(Vs, gv + (long)t * 64 * ldb, ldb);
        const long off = rowid * N + t * 64 + 4 * (l >> 4);
        f32x4 s[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) s[mt] = *reinterpret_cast<const f32x4*>(a.map + off + 16 * mt);
        if (a.thresh) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    s[mt][r] = fw_keep(key, (unsigned long long)off + 16 * mt + r, a.thresh) ? s[mt][r] * a.inv_keep : 0.f;
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) store_acc_T<T>(Ps, LDR, 16 * mt, 0, s[mt]);
        __syncthreads();
        // O^T[d][i] += sum_j V[j][d] A''[i][j]
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const uint4 pf = frag_kc(Ps, LDR, 0, c);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) mma_chunk<T>(o[dt], frag_km<T>(Vs, LDR, 16 * dt, c), pf);
        }
        __syncthreads();
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store_acc_T<T>(Os, LDR, 16 * dt, 0, o[dt]);
    wave_fence();
    store_rows16<T>(Os, a.out + (((long)b * N + qt * 64 + 16 * w) * a.ldo + h * 64) * SZ, a.ldo * SZ);
}

// dvec[row] = sum_j P[row][j] dA[row][j]; one wave per row of N
__global__ __launch_bounds__(NTH) void gattn_rowdotn_kernel(const float* __restrict__ P, const float* __restrict__ dA, float* __restrict__ dvec, int N) {
    const long row = (long)blockIdx.x * 4 + wave_id();
    const int l = lane_id();
    float s = 0.f;
    for (int j = 4 * l; j < N; j += 256) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(P + row * N + j), g = *reinterpret_cast<const f32x4*>(dA + row * N + j);
        s += p[0] * g[0] + p[1] * g[1] + p[2] * g[2] + p[3] * g[3];
    }
    s = wave_sum(s);
    if (l == 0) dvec[row] = s;
}

#define BN_PASS(RI, RO, CJ, EP, ...) \
    hipLaunchKernelGGL((bandsn_pass_kernel<RI, RO, CJ, EP>), dim3(N / 64, N / 64, (unsigned)maps), dim3(NTH), 0, st, __VA_ARGS__)
// map += filter(map) over B * heads maps; work: 4 planes per map (T^t re | im, X re | im), backward (pmap != nullptr) 6: the
// spectrum of P (re | im) behind them, against which the column pass reduces d lamb
static void launch_filtern(float* map, float* work, const float* pmap, const GAttnArgs& a, hipStream_t st) {
    const int N = a.N, maps = a.B * a.heads;
    const size_t per = (size_t)maps * N * N;
    float* Tr = work; float* Ti = work + per; float* Xr = work + 2 * per; float* Xi = work + 3 * per;
    const float* nf = nullptr;
    const unsigned char* nu = nullptr;
    if (pmap) {
        float* Qr = work + 4 * per; float* Qi = work + 5 * per;
        BN_PASS(true, false, false, E_PLAIN, pmap, nf, a.panels, Tr, Ti, N, 1.0f, nu, nf, nf, nf, (float*)nullptr, 0, 1, a.heads);
        BN_PASS(false, false, false, E_PLAIN, (const float*)Tr, (const float*)Ti, a.panels, Qr, Qi, N, 1.0f, nu, nf, nf, nf, (float*)nullptr, 0, 1, a.heads);
        BN_PASS(true, false, false, E_PLAIN, (const float*)map, nf, a.panels, Tr, Ti, N, 1.0f, nu, nf, nf, nf, (float*)nullptr, 0, 1, a.heads);
        BN_PASS(false, false, false, E_WEIGHT_DL, (const float*)Tr, (const float*)Ti, a.panels, Xr, Xi, N, 1.0f, a.bandidx, a.lamb, (const float*)Qr,
                (const float*)Qi, a.dlamb, a.nb, a.lamb_batch, a.heads);
    } else {
        BN_PASS(true, false, false, E_PLAIN, (const float*)map, nf, a.panels, Tr, Ti, N, 1.0f, nu, nf, nf, nf, (float*)nullptr, 0, 1, a.heads);
        BN_PASS(false, false, false, E_WEIGHT, (const float*)Tr, (const float*)Ti, a.panels, Xr, Xi, N, 1.0f, a.bandidx, a.lamb, nf, nf, (float*)nullptr,
                a.nb, a.lamb_batch, a.heads);
    }
    BN_PASS(false, false, true, E_PLAIN, (const float*)Xr, (const float*)Xi, a.panels, Tr, Ti, N, 1.0f, nu, nf, nf, nf, (float*)nullptr, 0, 1, a.heads);
    BN_PASS(false, true, true, E_PLAIN, (const float*)Tr, (const float*)Ti, a.panels, map, (float*)nullptr, N, 1.0f / ((float)N * (float)N), nu, nf, nf,
            nf, (float*)nullptr, 0, 1, a.heads);
}
template <typename T> static int bandsn_fwd(const GAttnArgs& a, float* work, hipStream_t st) {
    const int tiles = a.B * a.heads * (a.N / 64);
    hipLaunchKernelGGL((gattn_probsn_kernel<T>), dim3(tiles), dim3(NTH), (size_t)2 * GG<T>::TILE, st, a);
    launch_filtern(a.map, work, nullptr, a, st);
    hipLaunchKernelGGL((gattn_applyn_kernel<T>), dim3(tiles), dim3(NTH), (size_t)3 * GG<T>::TILE, st, a);
    FW_LAUNCH_RET();
}
template <typename T> static int bandsn_bwd(const GAttnArgs& a, float* work, hipStream_t st) {
    const int maps = a.B * a.heads, tiles = maps * (a.N / 64);
    const size_t lds_rows = (size_t)4 * GG<T>::TILE, lds = bwd_lds<T>(false);
    FW_SET_LDS_ONCE((gattn_dc_rows_kernel<T, true, 0>), lds_rows);
    hipLaunchKernelGGL((gattn_dc_rows_kernel<T, true, 0>), dim3(tiles), dim3(NTH), lds_rows, st, a);
    launch_filtern(a.map2, work, a.pmap, a, st);
    hipLaunchKernelGGL(gattn_rowdotn_kernel, dim3(maps * (a.N / 4)), dim3(NTH), 0, st, (const float*)a.pmap, (const float*)a.map2, a.dvec, a.N);
    FW_SET_LDS_ONCE((gattn_maps_bwd_kernel<T, 0>), lds);
    hipLaunchKernelGGL((gattn_maps_bwd_kernel<T, 0>), dim3(tiles), dim3(NTH), lds, st, a);
    FW_LAUNCH_RET();
}
template <typename T> static int dispatch(const GAttnArgs& a, bool bwd, hipStream_t st) {
    const bool lamb = a.lamb != nullptr;
    if (a.N == 64) {
        if (lamb) bwd ? launch_bwd<T, 1, true>(a, st) : launch_fwd<T, 1, true>(a, st);
        else bwd ? launch_bwd<T, 1, false>(a, st) : launch_fwd<T, 1, false>(a, st);
    } else if (a.N != 256) {
        if (lamb) launch_stream_dc<T>(a, bwd, st);                     // common_ok: 'DC' at N = 576 / 1024 only
        else launch_stream<T>(a, bwd, st);
    } else if (lamb) {
        bwd ? launch_dc_bwd<T>(a, st) : launch_dc_fwd<T>(a, st);
    } else {
        bwd ? launch_bwd<T, 4, false>(a, st) : launch_fwd<T, 4, false>(a, st);
    }
    FW_LAUNCH_RET();
}
// lamb: N = 64 with the 64x64 tables (any nb), or N in {256, 576, 1024} in the 'DC' form (nb = 2, band 0 = bin (0, 0): no tables);
// nothing else has a kernel
// N: 64 and 256 (register kernels), or any other multiple of 64 in [128, 1024] (streaming forward; lamb at 576 and 1024 only)
static bool common_ok(const GAttnArgs& a, int dtype) {
    const int sz = dtype == FW_DT_BF16 ? 2 : 4;
    const bool stream_n = a.N % 64 == 0 && a.N >= 128 && a.N <= 1024 && (!a.lamb || a.N == 576 || a.N == 1024);
    if (!(a.q && a.k && a.v && a.lse && a.B > 0 && a.heads > 0 && (a.N == 64 || a.N == 256 || stream_n))) return false;
    if ((a.ld * sz) % 16 || ((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v) % 16) return false;
    if (a.thresh && !a.seed) return false;
    if (a.lamb) {
        if (!(a.nb >= 1 && a.nb <= 16 && (a.lamb_batch == 1 || a.lamb_batch == a.B))) return false;
        if (a.N == 64 ? !(a.bandidx && a.panels) : !(a.nb == 2 && !a.bandidx && !a.panels)) return false;
    }
    return true;
}
// <n>_bands on the N x N map, N in {256, 576, 1024}: the tables are required (that is what tells it from the table-free 'DC' form of
// fw_gattn_fwd); the tiled passes put the maps on the grid's z axis
static bool bands_ok(const GAttnArgs& a, int dtype) {
    const int sz = dtype == FW_DT_BF16 ? 2 : 4;
    if (!(a.N == 256 || ((a.N == 576 || a.N == 1024) && (long)a.B * a.heads <= 65535))) return false;
    if (!(a.q && a.k && a.v && a.lse && a.B > 0 && a.heads > 0)) return false;
    if ((a.ld * sz) % 16 || ((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v) % 16) return false;
    if (a.thresh && !a.seed) return false;
    return a.lamb && a.bandidx && a.panels && (uintptr_t)a.panels % 16 == 0 && (uintptr_t)a.bandidx % 4 == 0 && a.nb >= 1 && a.nb <= 16 &&
           (a.lamb_batch == 1 || a.lamb_batch == a.B);
}
template <typename T> static int bands_dispatch(const GAttnArgs& a, float* work, bool bwd, hipStream_t st) {
    if (a.N == 256) return bwd ? bands_bwd<T>(a, work, st) : bands_fwd<T>(a, work, st);
    return bwd ? bandsn_bwd<T>(a, work, st) : bandsn_fwd<T>(a, work, st);
}
// what the four entries share: operands, geometry, Dropout, lamb and its tables
static GAttnArgs common_args(const void* q, const void* k, const void* v, long ld, int B, int heads, int N, float scale, const void* seed,
                             int site, float drop_p, const float* lamb, int nb, int lamb_batch, const void* bandidx, const float* panels) {
    GAttnArgs a{};
    a.q = (const char*)q; a.k = (const char*)k; a.v = (const char*)v; a.ld = ld;
    a.B = B; a.heads = heads; a.N = N; a.scale = scale;
    a.seed = (const unsigned*)seed; a.site = (unsigned)site; a.thresh = drop_p > 0.f ? fw_drop_thresh(drop_p) : 0u;
    a.inv_keep = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
    a.lamb = lamb; a.nb = nb; a.lamb_batch = lamb_batch; a.bandidx = (const unsigned char*)bandidx; a.panels = panels;
    return a;
}
}  // namespace

extern "C" int fw_gattn_fwd(int dtype, const void* q, const void* k, const void* v, long ld, void* out, long ldo, float* lse, int B, int heads,
                            int N, float scale, const void* seed, int site, float drop_p, const float* lamb, int nb, int lamb_batch,
                            const void* bandidx, const float* panels, void* stream) {
    GAttnArgs a = common_args(q, k, v, ld, B, heads, N, scale, seed, site, drop_p, lamb, nb, lamb_batch, bandidx, panels);
    a.out = (char*)out; a.ldo = ldo; a.lse = lse;
    const int sz = dtype == FW_DT_BF16 ? 2 : 4;
    FW_CHECK_ARG(dtype == FW_DT_BF16 || dtype == FW_DT_F32);
    FW_CHECK_ARG(common_ok(a, dtype) && out && (ldo * sz) % 16 == 0 && (uintptr_t)out % 16 == 0 && drop_p >= 0.f && drop_p < 1.f);
    return dtype == FW_DT_BF16 ? dispatch<bf16raw>(a, false, (hipStream_t)stream) : dispatch<float>(a, false, (hipStream_t)stream);
}

extern "C" int fw_gattn_bwd(int dtype, const void* q, const void* k, const void* v, long ld, const void* o, long ldo, const void* dout, long lddo,
                            const float* lse, float* dvec, void* dq, void* dk, void* dv, long ldd, int B, int heads, int N, float scale,
                            const void* seed, int site, float drop_p, const float* lamb, float* dlamb, int nb, int lamb_batch,
                            const void* bandidx, const float* panels, void* stream) {
    GAttnArgs a = common_args(q, k, v, ld, B, heads, N, scale, seed, site, drop_p, lamb, nb, lamb_batch, bandidx, panels);
    a.o = (const char*)o; a.ldo = ldo;
    a.dout = (const char*)dout; a.lddo = lddo; a.lse = const_cast<float*>(lse); a.dvec = dvec;
    a.dq = (char*)dq; a.dk = (char*)dk; a.dv = (char*)dv; a.ldd = ldd; a.dlamb = dlamb;
    const int sz = dtype == FW_DT_BF16 ? 2 : 4;
    FW_CHECK_ARG(dtype == FW_DT_BF16 || dtype == FW_DT_F32);
    FW_CHECK_ARG(common_ok(a, dtype) && o && dout && dq && dk && dv && (lamb ? dlamb != nullptr : dvec != nullptr));
    FW_CHECK_ARG(!(lamb && N != 64) || dvec != nullptr);                   // the DC form keeps rowsum(P G) there
    FW_CHECK_ARG((ldo * sz) % 16 == 0 && (lddo * sz) % 16 == 0 && (ldd * sz) % 16 == 0 && drop_p >= 0.f && drop_p < 1.f);
    FW_CHECK_ARG(((uintptr_t)o | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) % 16 == 0);
    return dtype == FW_DT_BF16 ? dispatch<bf16raw>(a, true, (hipStream_t)stream) : dispatch<float>(a, true, (hipStream_t)stream);
}

// <n>_bands with N x N masks at N = 256 / 576 / 1024 (see fwair.h): probs -> the filter passes of that N -> apply
extern "C" int fw_gattn_bands_fwd(int dtype, const void* q, const void* k, const void* v, long ld, void* out, long ldo, float* lse, int B, int heads,
                                  int N, float scale, const void* seed, int site, float drop_p, const float* lamb, int nb, int lamb_batch,
                                  const void* bandidx, const float* panels, float* amap, float* work, void* stream) {
    GAttnArgs a = common_args(q, k, v, ld, B, heads, N, scale, seed, site, drop_p, lamb, nb, lamb_batch, bandidx, panels);
    a.out = (char*)out; a.ldo = ldo; a.lse = lse; a.map = amap;
    const int sz = dtype == FW_DT_BF16 ? 2 : 4;
    FW_CHECK_ARG(dtype == FW_DT_BF16 || dtype == FW_DT_F32);
    FW_CHECK_ARG(bands_ok(a, dtype) && out && amap && work && (ldo * sz) % 16 == 0 && drop_p >= 0.f && drop_p < 1.f);
    FW_CHECK_ARG(((uintptr_t)out | (uintptr_t)amap | (uintptr_t)work) % 16 == 0);
    return dtype == FW_DT_BF16 ? bands_dispatch<bf16raw>(a, work, false, (hipStream_t)stream) : bands_dispatch<float>(a, work, false, (hipStream_t)stream);
}

extern "C" int fw_gattn_bands_bwd(int dtype, const void* q, const void* k, const void* v, long ld, const void* dout, long lddo, const float* lse,
                                  float* dvec, void* dq, void* dk, void* dv, long ldd, int B, int heads, int N, float scale, const void* seed,
                                  int site, float drop_p, const float* lamb, float* dlamb, int nb, int lamb_batch, const void* bandidx,
                                  const float* panels, const float* amap, float* pmap, float* gmap, float* work, void* stream) {
    GAttnArgs a = common_args(q, k, v, ld, B, heads, N, scale, seed, site, drop_p, lamb, nb, lamb_batch, bandidx, panels);
    a.dout = (const char*)dout; a.lddo = lddo; a.lse = const_cast<float*>(lse); a.dvec = dvec;
    a.dq = (char*)dq; a.dk = (char*)dk; a.dv = (char*)dv; a.ldd = ldd; a.dlamb = dlamb;
    a.map = const_cast<float*>(amap); a.pmap = pmap; a.map2 = gmap;
    const int sz = dtype == FW_DT_BF16 ? 2 : 4;
    FW_CHECK_ARG(dtype == FW_DT_BF16 || dtype == FW_DT_F32);
    FW_CHECK_ARG(bands_ok(a, dtype) && dout && dq && dk && dv && dvec && dlamb && amap && pmap && gmap && work);
    FW_CHECK_ARG((lddo * sz) % 16 == 0 && (ldd * sz) % 16 == 0 && drop_p >= 0.f && drop_p < 1.f);
    FW_CHECK_ARG(((uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv | (uintptr_t)amap | (uintptr_t)pmap | (uintptr_t)gmap | (uintptr_t)work) % 16 == 0);
    return dtype == FW_DT_BF16 ? bands_dispatch<bf16raw>(a, work, true, (hipStream_t)stream) : bands_dispatch<float>(a, work, true, (hipStream_t)stream);
}
