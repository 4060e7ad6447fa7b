/* fwair.h -- C ABI of libfwair_hip.so: the MI355X (gfx950) kernels behind the AirNet training hot path.
 *
 * The reference (stcodeer/Frequency-wised_All-in-One_Image_Restoration_Model) is pure eager PyTorch; it
 * has no native ABI.  Each entry point below replaces the PyTorch operator sequence cited next to it
 * (file:line relative to the reference root).  The Python host (net/model.py ... in the package
 * directory) binds these through ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain pointers and sizes only; every device buffer is owned by the caller (PyTorch allocator);
 *     the library never allocates, frees or retains device memory and never synchronises the device;
 *   - `dtype`: 0 = f32, 1 = bf16 ("T" below) -- the storage type of activations / GEMM operands;
 *     accumulation, the residual stream, statistics, losses, parameters and gradients are f32;
 *   - leading dimensions (`ld*`) are in ELEMENTS; rows are tokens (b, y, x) in raster order;
 *   - `stream` is a hipStream_t; every function is re-entrant and takes its stream per call;
 *   - return value: 0 ok, < 0 argument / shape error (the negated source line), > 0 a hipError_t.
 */
#ifndef FWAIR_H
#define FWAIR_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- GEMM: C[m][n] = epi(alpha * sum_k X(m,k) W(n,k)) ------------------------------------------------
 * nn.Linear forward/backward: net/decoder_Uformer.py:98-125 (to_q/to_kv), :294 (proj),
 * net/utils/leff.py:100,114 (linear1/linear2), net/encoder_Uformer.py:942,954-956 (heads); with
 * fw_im2col4 / fw_pixel_shuffle also Conv2d k4s2p1 and ConvTranspose2d k2s2 (decoder_Uformer.py:414-449).
 * x_trans / w_trans = 1: the operand is stored reduction-major (element (i,k) at k*ld + i).
 * x_op / w_op = 1: GELU applied to the operand while it is staged (leff.py:100,106 activations).
 * act: 0 none, 1 LeakyReLU(slope), 2 multiply by GELU'(aux[m][n]), 3 GELU.
 * epilogue order: alpha, +bias[n], act, *rowscale[m / rows_per_scale] (DropPath), +residual[m][n] (f32).
 * out_f32: C is f32 (else T).  accumulate: atomicAdd into f32 C (required when splitk > 1).
 * C2 (optional, T): second output GELU(v) (LeFF keeps pre- and post-activation).  xsum (optional, x_trans only):
 * xsum[m] += sum_k X(m,k), i.e. the bias gradient falls out of the weight-gradient GEMM. */
int fw_gemm(int dtype, const void* X, long ldx, int x_trans, int x_op, const void* W, long ldw, int w_trans, int w_op,
            void* C, long ldc, int out_f32, int accumulate, int M, int N, int K, float alpha, const float* bias, int act,
            float slope, const void* aux, long ldaux, const float* rowscale, int rows_per_scale, const float* residual,
            long ldr, int splitk, void* C2, long ldc2, float* xsum, long c_zstride, long xsum_zstride, void* stream);
/* Measurement aid: the kernel the calling thread's last fw_gemm was dispatched to, by name: copies the launched kernel's name into buf (rocprofv3's demangled spelling without spaces and with
 * "unsigned short" written bf16, e.g. "gemm_ring_kernel<bf16,128,2,true>"); returns its length, -1 on a bad buffer. */
int fw_gemm_last_kernel(char* buf, int n);

/* Every weight gradient dW = dY^T x of a backward pass in ONE launch (bf16 operands, both token-major; f32 dW): the host queues the
 * products nobody reads before the optimizer step and hands over a table.  tab: device int64 [nprob][16] = {dY, x, dW, ld(dY), ld(x),
 * ld(dW), rows of dW, columns of dW, tokens, tokens per slice (multiple of 32), slices, db (f32, or 0), c_zstride, xsum_zstride,
 * accumulate, 0};  probs: device scratch, nprob * fw_wgrad_group_prob_bytes() bytes;  items: device int32 [nitems][4] = {problem,
 * row tile, column tile, slice} in units of `tile` = 128 (4-wave workgroups) or 256 (8 waves: half the operand bytes per FLOP).  One slice: the tile adds into dW; several: slice z stores its partial tile at
 * dW + z * c_zstride (fold with fw_slab_reduce_multi).  Replaces nn.Linear's weight / bias gradients of decoder_Uformer.py:98-125,294,
 * leff.py:100,114 and the encoder's, as fw_gemm(x_trans = w_trans = 1) does one product at a time. */
int fw_wgrad_group_prob_bytes(void);
int fw_wgrad_group(const void* tab, void* probs, int nprob, const void* items, int nitems, int tile, void* stream);

/* split-K without atomics: slice z stores its partial tile at C + z*c_zstride (and xsum + z*xsum_zstride); this sums the slices.
 * accumulate: 0 store, 1 add (a long z range may be split over blocks that add atomically), 2 add with the whole z range in one block
 * (one read-modify-write per address: deterministic) */
int fw_slab_reduce(const float* slab, int nz, long n, long zstride, float* dst, int accumulate, float* dst2, long off2, long n2,
                   void* stream);
/* Many slabs in one launch (ops.flush_slabs: every weight-gradient / LayerNorm partial of a backward pass is folded once,
 * at its end).  tab: device int64 [num][12] = slab, dst, dst2, n, zstride, off2, n2, nz, zper, nchunks, upw, atomics; prefix: device
 * int64 [num + 1] block offsets (entry e owns ceil(nchunks * ceil(nz / zper) / (4 * upw)) blocks of 4 waves; a wave folds upw
 * units of 64 columns x zper slab rows).  Every entry ACCUMULATES into dst / dst2. */
int fw_slab_reduce_multi(const void* tab, const void* prefix, int num, long total_blocks, void* stream);

/* ---- LayerNorm over the f32 stream -> T (decoder_Uformer.py:567,594,666,744; encoder_Uformer.py:941) -- */
int fw_layernorm_fwd(int dtype, const float* x, long ldx, const float* gamma, const float* beta, void* y, long ldy,
                     float* mean, float* rstd, int rows, int C, float eps, void* stream);
/* dx = (dres?) + LN'(dy); dgamma, dbeta accumulated.  partial: caller scratch f32 [fw_layernorm_bwd_blocks(rows, C)][2*C]
 * for the per-block column sums (folded with fw_slab_reduce instead of thousands of same-address atomics). */
int fw_layernorm_bwd_blocks(int rows, int C);
int fw_layernorm_bwd(int dtype, const void* dy, long lddy, const float* x, long ldx, const float* gamma, const float* mean,
                     const float* rstd, const float* dres, long lddres, float* dx, long lddx, float* dgamma, float* dbeta,
                     float* partial, int rows, int C, void* stream);
/* Same, plus an optional second output twin[rows][ldtw] (type T) = dx * twscale[row / tw_rows_per_scale]: the DropPath-scaled
 * operand copy that the backward of the Linear feeding this residual stream needs (saves its separate cast kernel). */
int fw_layernorm_bwd2(int dtype, const void* dy, long lddy, const float* x, long ldx, const float* gamma, const float* mean,
                      const float* rstd, const float* dres, long lddres, float* dx, long lddx, float* dgamma, float* dbeta,
                      float* partial, int rows, int C, void* twin, long ldtw, const float* twscale, int tw_rows_per_scale,
                      void* stream);
/* Same, with dy taken either as T [rows][lddy] (dy_slab == NULL: exactly fw_layernorm_bwd2) or straight from the unfolded slab of the
 * split-K input-gradient GEMM in front: dy_slab f32, 16-byte aligned, nz slices zstride floats apart (zstride >= rows * C, a multiple
 * of 4), each rows x C contiguous partials; dy / lddy are then not read.  A lane sums its vector over the slices in the association
 * fw_slab_reduce uses with its whole z range in one block -- partial sums of slices j, j + 4, ... for j = 0..3, total
 * s0 + ((s1 + s2) + s3) -- and rounds it to T as fw_cast_rows does (no rounding for T = f32), so dx and twin are bit for bit those of
 * fw_slab_reduce(accumulate 0) -> fw_cast_rows -> fw_layernorm_bwd2, and dgamma / dbeta see the same dy, without the two launches and
 * the f32 and T round trips between them.
 * All three entries fold a workgroup's column partials through LDS in a fixed order: one (rows, C) gives the same `partial` bits on
 * every call. */
int fw_layernorm_bwd_slab(int dtype, const void* dy, long lddy, const float* dy_slab, int nz, long zstride, const float* x, long ldx,
                          const float* gamma, const float* mean, const float* rstd, const float* dres, long lddres, float* dx,
                          long lddx, float* dgamma, float* dbeta, float* partial, int rows, int C, void* twin, long ldtw,
                          const float* twscale, int tw_rows_per_scale, void* stream);

/* ---- learnable window modulator of the decoder blocks (--learnable_modulator; decoder_Uformer.py:536-539,687-691) ----------
 * The reference adds an nn.Embedding(64, C) table to the 64 tokens of every 8x8 window after norm1, the cyclic shift and the window
 * partition, in front of the Q/K/V projection.  On the token-major [B*H*W, C] stream the window position of row r = (b, yy, xx)
 * under shift s (0 or 4) is  p(r) = ((yy - s) mod 8) * 8 + ((xx - s) mod 8)  (roll(-s) moves pixel yy to rolled row (yy - s) mod H,
 * and 8 | H, 8 | W).
 * fw_layernorm_mod_fwd: y[r] = T(LN(x[r]) * gamma + beta + mod[p(r)]); mod f32 [64][C], 16-byte aligned; mean / rstd exactly as
 * fw_layernorm_fwd writes them (the same kernel body with the table add compiled in).
 * fw_modulator_bwd: dmod[p] += sum over the rows with p(r) = p of dy[r]  (dmod f32 [64][C], ACCUMULATED).  dy is read once; the
 * rows / 64 terms of a sum are cut into fw_modulator_bwd_blocks(rows, C) slices, slice z stores partial[z] (caller scratch f32
 * [slices][64][C], 16-byte aligned) with plain stores, and fw_slab_reduce (accumulate = 2: one read-modify-write per address) folds
 * them into dmod on the same stream: no floating-point atomics, identical calls give identical bits.  dmod == NULL leaves the fold
 * to the caller (ops.flush_slabs folds every slab of a backward pass in one launch).  LayerNorm's own backward is unchanged: the
 * gradient reaching it is the same dy. */
int fw_layernorm_mod_fwd(int dtype, const float* x, long ldx, const float* gamma, const float* beta, const float* mod, void* y,
                         long ldy, float* mean, float* rstd, int rows, int C, int H, int W, int shift, float eps, void* stream);
int fw_modulator_bwd_blocks(int rows, int C);
int fw_modulator_bwd(int dtype, const void* dy, long lddy, float* dmod, float* partial, int rows, int C, int H, int W, int shift,
                     void* stream);

/* ---- window attention (decoder_Uformer.py:240-293 with :387-409,634-651,678-686,721-729 folded in;
 *      encoder_Uformer.py:152-183 "origin", :256-310 intra / inter band attention) ---------------------
 * q/k/v: T rows = tokens of B*L images of H x W, head h at column h*D; D in {56, 28}, or {32, 64}
 * (decoder at --embed_dim 32 / 64 and the ViT body: mode 0, nkt 1, any lfs; D = 32 is not taken with mode 1).
 * L: bands (1 for the decoder); mode 0: keys = the query's own band, 1: keys = the other L-1 bands (nkt = L-1).
 * bias: f32 [L*L][225][heads] relative-position tables; shift: cyclic shift (0 or 4).
 * lfs: 0 none; 1 P' = a P + b; 2 P' = a P + b + c B1(P) with coef f32 [B][heads][3] = (a,b,c) and lfs_tab the
 * DFT panels of fw_attn_lfs_table_elems() T elements followed by the f32 mask [48][32] (host: fwair/lfs.py).
 * lse: f32 [B*nW*L*heads][64] log-sum-exp saved for the backward pass. */
int fw_attn_lfs_table_elems(void);
int fw_attn_fwd(int dtype, int D, int nkt, int lfs, const void* q, const void* k, const void* v, long ld, void* out, long ldo,
                float* lse, const float* bias, const float* coef, const void* lfs_tab, int B, int H, int W, int heads, int L,
                int mode, int shift, float scale, void* stream);
/* dbias: f32 [L*L][225][heads] (layout of `bias`); dcoef: f32 [B][heads][3]; both accumulated.  dk2/dv2: second slot of
 * key gradients when nkt == 2 (each key band is attended by two query bands).  dq_pad: columns behind the last head's dq columns
 * that are written too, with zeros (0, or roundup(heads*D, 8) - heads*D when dq | pad | dk | dv share one buffer: the pad then
 * holds defined values and the buffer can be one GEMM operand). */
int fw_attn_bwd(int dtype, int D, int nkt, int lfs, const void* q, const void* k, const void* v, long ld, const void* out,
                long ldo, const void* dout, long lddo, const float* lse, const float* bias, const float* coef,
                const void* lfs_tab, void* dq, void* dk, void* dv, void* dk2, void* dv2, long ldd, float* dbias,
                float* dcoef, int B, int H, int W, int heads, int L, int mode, int shift, float scale, int dq_pad, void* stream);
/* grid.x of the launch fw_attn_fwd (backward = 0) / fw_attn_bwd (1) makes for a problem of nwin = B * (H/8) * (W/8) windows: every
 * (head, band) is walked in that many contiguous window ranges of ceil(nwin / grid.x) windows (the last ones may be short or empty).
 * It is 256 CUs times the workgroups of the chosen kernel one CU holds -- bounded by its LDS bytes and its compiled register
 * count, as the runtime reports them -- over heads * L, clamped to [1, nwin].  nkt 1: mode 0; nkt 2: the inter-band form over
 * L = 3.  Negative: argument error, or a combination served by the kernels that do not walk by this rule (mode 1 over two bands:
 * forward one workgroup per item up to 4096, backward 1024 / (heads * L) ranges).  dbias receives one atomic addition per busy
 * workgroup and dcoef one per wave of every workgroup holding windows of the image, so their summation ORDER follows this figure;
 * out, lse, dq, dk, dv do not depend on it.  Not to be called inside a stream capture. */
int fw_attn_chunks(int dtype, int D, int nkt, int lfs, int backward, int nwin, int heads, int L);

/* ---- LeFF depthwise 3x3 (net/utils/leff.py:104-111).
 * fwd: h2 = dwconv(GELU?(in)) + bias, g2 = GELU(h2).  in_gelu = 1: `in` is the PRE-activation h1 of linear1 and its GELU (leff.py:100) is
 * evaluated as the input tile is staged -- the activation g1 = GELU(h1) is then never written to HBM; in_gelu = 0: `in` is g1.
 * bwd: dh1 = GELU'(h1) * convT(dh2), dw / dbias accumulated; g1 may be NULL: the weight gradient then takes GELU(h1) in-kernel
 * (input-centric form: exactly one GELU per element).
 * w is TAP-MAJOR f32 [9][C] (a per-step permuted copy of the [C,1,3,3] parameter); dw is ACCUMULATED into in the
 * parameter's own [C][9] layout, dbias likewise ([C]).  h2, g2 and dh1 are plain stores.
 * Checked: C and every row stride a multiple of 8 (bf16) / 4 (f32) elements, every row stride >= C, W % 8 == 0, ldg == ld1 (g1, h1
 * and dh2 share one row stride), sizes > 0. */
int fw_dwconv_fwd(int dtype, const void* in, long ld1, int in_gelu, const float* w, const float* bias, void* h2, void* g2, long ld2, int B,
                  int H, int W, int C, void* stream);
int fw_dwconv_bwd(int dtype, const void* dh2, long ldg, const void* g1, const void* h1, long ld1, const float* w, void* dh1,
                  long ldo, float* dw, float* dbias, int B, int H, int W, int C, void* stream);

/* ---- Downsample conv k4 s2 p1 (decoder_Uformer.py:414-430) as GEMM: K order (ky, kx, ci) -------------- */
int fw_im2col4(int dtype, const float* x, long ldx, void* col, int B, int H, int W, int C, void* stream);
int fw_col2im4(int dtype, const void* dcol, float* dx, long lddx, const float* dres, long ldr, int B, int H, int W, int C,
               void* stream);
/* ---- Upsample convT k2 s2 (decoder_Uformer.py:434-449) = Linear(Cin -> 4 Cout) + depth-to-space ------- */
int fw_pixel_shuffle(int dtype, const void* g, const float* bias, float* out, long ldo, int B, int H, int W, int Cout,
                     void* stream);
int fw_pixel_unshuffle(int dtype, const float* dout, long ldo, void* dg, int B, int H, int W, int Cout, void* stream);
int fw_colsum(int x_dtype, const void* x, long ldx, float* out, long rows, int cols, void* stream);

/* ---- InputProj 3x3 conv 3->C + LeakyReLU(0.01) (decoder_Uformer.py:453-472), NCHW f32 image -----------
 * fwd: C % 4 == 0, C <= 1024, ldo % 4 == 0, out and bias 16-byte aligned.  bwd: any C and any strides (16-byte loads when C, ldo,
 * ldy are multiples of 4 and out / dy are 16-byte aligned, one channel per lane otherwise); dw / db are accumulated into. */
int fw_inproj_fwd(const float* img, const float* w, const float* bias, float* out, long ldo, int B, int H, int W, int C,
                  float slope, void* stream);
int fw_inproj_bwd(const float* img, const float* out, long ldo, const float* dy, long ldy, float* dw, float* db, int B, int H,
                  int W, int C, float slope, void* stream);
/* ---- OutputProj 3x3 conv C->3 + global residual x + y (decoder_Uformer.py:476-499,1171) ---------------
 * C % 4 == 0, ldf % 4 == 0, lddf % 4 == 0, fea / dfea 16-byte aligned; fwd: C <= 896 (weight fragments + product tile in LDS),
 * bwd: C <= 1024; dw / db are accumulated into, dfea is overwritten.  img may be null (no residual). */
int fw_outproj_fwd(const float* fea, long ldf, const float* w, const float* bias, const float* img, float* out, int B, int H,
                   int W, int C, void* stream);
int fw_outproj_bwd(const float* dout, const float* fea, long ldf, const float* w, float* dfea, long lddf, float* dw, float* db,
                   int B, int H, int W, int C, void* stream);

/* ---- casts / copies / re-layouts ------------------------------------------------------------------ */
int fw_cast_rows(int dtype, const float* src, long lds_, void* dst, long ldd, long rows, int cols, const float* rowscale,
                 int rows_per_scale, void* stream);
int fw_copy_rows(const float* src, long lds_, float* dst, long ldd, long rows, int cols, int accumulate, void* stream);
int fw_add_rows(int dtype, const void* src, long lds_, void* dst, long ldd, long rows, int cols, void* stream);
int fw_cast_flat(int dtype, const float* src, void* dst, long n, void* stream);
int fw_permute3(int in_dtype, int out_dtype, const void* in, void* out, int d0, int d1, int d2, long s0, long s1, long s2,
                int accumulate, void* stream);
/* `num` re-layouts of the fw_permute3 kind (f32 source) in one launch: the per-step operand copies of parameters (functional.shadow:
 * depthwise taps, k4s2 / k2s2 convolution weights, bf16 rows that are not 16-byte aligned).  tab: device int64 [num][10] =
 * {src, dst, d0, d1, d2, s0, s1, s2, out_is_bf16, 0}; prefix: device int64 [num + 1] block offsets, entry e owning
 * ceil(d0*d1*d2 / 1024) blocks. */
int fw_permute3_multi(const void* tab, const void* prefix, int num, long total_blocks, void* stream);
int fw_fill(float* p, long n, float v, void* stream);
/* LeakyReLU on a contiguous f32 vector -> T, and its backward (encoder_Uformer.py:953-957 head MLPs) */
int fw_lrelu_fwd(int dtype, const float* x, void* y, long n, float slope, void* stream);
int fw_lrelu_bwd(int dtype, const void* dy, const float* x, float* dx, long n, float slope, void* stream);

/* ---- losses (train.py:88-92): loss accumulated into *loss; gradient scaled by gscale ----------------- */
int fw_l1_loss(const float* a, const float* b, float* da, long n, float gscale, float* loss, void* stream);
int fw_ce0_loss(const float* logits, float* dlogits, int R, int N, float gscale, float* loss, void* stream);
/* Structural similarity of the restoration a and the clean image b, both f32 [n][C][H][W] contiguous, 8 <= H, W <= 1024
 * (utils/pytorch_ssim/__init__.py:19-43: Gaussian 11x11 window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2, mean over the map):
 * *loss += mean S(a, b); with da != NULL, da (+)= gscale * d mean(S) / d a -- `+=` when accumulate is set, `=` otherwise -- so the term
 * -w (1 - SSIM) joins the gradient fw_l1_loss stored, stream-ordered after it.  One launch; every da element is written by one thread
 * (bit-reproducible), the value takes one float atomic per workgroup. */
int fw_ssim11_loss(const float* a, const float* b, float* da, int n, int C, int H, int W, float gscale, int accumulate, float* loss,
                   void* stream);

/* ---- Adam (train.py:63,96; torch.optim.Adam defaults) and MoCo EMA (net/utils/moco.py:44-50) ----------
 * hyper: device f32[4] = {lr, beta1^t, beta2^t, t}; fw_adam_tick advances t so graphs replay correctly. */
int fw_adam_tick(float* hyper, float b1, float b2, void* stream);
int fw_adam(int shadow_dtype, float* p, const float* g, float* m, float* v, void* shadow, long n, const float* hyper, float b1,
            float b2, float eps, void* stream);
int fw_ema(int shadow_dtype, float* pk, const float* pq, void* shadow, long n, float momentum, void* stream);

/* ---- image band decomposition (net/utils/frequency_decompose.py:28-118) ------------------------------ */
int fw_dft2_fwd(const float* img, float* fr, float* fi, int nimg, int N, void* stream);
int fw_dft2_bands(const float* fr, const float* fi, const float* mask_unshifted, float* out, int nimg, int N, int nbands,
                  int mode, void* stream);
/* The same decomposition in ONE launch on the f32 MFMA for band masks that partition the spectrum (the encoder's pre-processing,
 * encoder_Uformer.py:964-966 / frequency_decompose.py:70-107), N = 64 or 128: out[b] = Re IDFT2(mask_b . DFT2(img)) for b < nbands - 1,
 * out[nbands-1] = img - the others.  panels: f32 [3][N][N] = cos, sin, -sin of 2 pi u i / N; dc_bits: bit b set = band b is the DC bin
 * alone (written as the image mean, no transform). */
int fw_dft2_decompose(const float* img, const float* mask, const float* panels, float* out, int nimg, int N, int nbands, int dc_bits,
                      void* stream);
/* Last band of a decomposition whose masks sum to one: out[nbands-1] = img - sum of the first nbands-1 bands of out
 * ([nbands][nimg][N][N], filled by fw_dft2_bands called with nbands-1).  Saves one masked inverse transform per image. */
int fw_band_residual(const float* img, float* out, int nimg, int N, int nbands, void* stream);
int fw_dc_split(const float* img, float* out, int nimg, int NN, void* stream);
/* The same three roles for maps larger than one CU's LDS (--patch_size 384 / 512; frequency_decompose.py:28-118 at those sizes):
 * square maps, N a multiple of 64 in [192, 512] (256 included, for comparison with the entries above), as passes of tiled f32-MFMA
 * products over the caller's work buffer.  panels as for fw_dft2_decompose.  No global state; every launch goes to `stream`.
 *   fw_dft2t_fwd        replaces torch.fft.fft2 (frequency_decompose.py:28-32): the contract of fw_dft2_fwd.
 *                       work: 2 * nimg * N * N floats.
 *   fw_dft2t_bands      replaces the mask / ifft2 loop (frequency_decompose.py:47-60,70-118): the contract of fw_dft2_bands.
 *                       mode 0 work: 2 * nbands * nimg * N * N floats; modes 1 and 2 read neither work nor panels (may be NULL).
 *   fw_dft2t_decompose  replaces the whole frequency_decompose_1 pre-processing (encoder_Uformer.py:964-966): the contract of
 *                       fw_dft2_decompose, dc_bits included.  work: (2 + 2 * nbands) * nimg * N * N floats. */
int fw_dft2t_fwd(const float* img, const float* panels, float* work, float* fr, float* fi, int nimg, int N, void* stream);
int fw_dft2t_bands(const float* fr, const float* fi, const float* mask_unshifted, const float* panels, float* work, float* out,
                   int nimg, int N, int nbands, int mode, void* stream);
int fw_dft2t_decompose(const float* img, const float* mask, const float* panels, float* work, float* out, int nimg, int N,
                       int nbands, int dc_bits, void* stream);
/* Band statistics of the spectrum of maps of ANY size (csrc/fw_spec.hip; utils/visualization_utils.py:158-184 and restore.py's
 * --band_report): out[n][b] = sum over the bins (u, v) with ring[u][v] == b of |F_n[u][v]| (power 0) or |F_n[u][v]|^2 (power 1),
 * F_n = the un-normalised DFT2 of map n.  8 <= H <= 1024 and 8 <= W <= 1024, independent, any value (odd, W % 4 != 0);
 * 1 <= nbands <= 32; nimg <= 65535; anything else is the argument error and nothing is launched.  Rows have pitch W exactly.
 *   src_kind 0  src = f32 [nimg][H][W]                                   (clean unused, may be NULL)
 *            1  src = u8  [nimg][H][W], the value 0..255 as a float      (clean unused, may be NULL)
 *            2  src = restored f32 [nimg][H][W], clean = u8 [nimg][H][W]: the map is clamp(restored, 0, 1) - clean / 255, the
 *               difference fw_eval_blend squares for the PSNR; it is formed in the first pass's loader, never written
 *   ring      u8 [H][W], UN-shifted coordinates (bin (0, 0) is DC), shared by all maps: the band of every bin; 255, or any value
 *             >= nbands, = the bin is in no band
 *   panels_h  f32 [3][Hp][Hp], panels_w f32 [3][Wp][Wp], Hp = 64 ceil(H / 64), Wp = 64 ceil(W / 64): cos, sin, -sin of
 *             2 pi i j / H (resp. W) at [i][j] for i, j < H (resp. W), ZERO elsewhere; 16-byte aligned
 *   work      f32, nimg * (2 * Hp * Wh + (Hp / 64) * (Wh / 64) * nbands) floats with Wh = 64 ceil((W / 2 + 1) / 64) (integer W / 2: the
 *             maps are real, so only the columns v <= W / 2 of the spectrum are computed and each stands for its mirror bin too);
 *             16-byte aligned; need not be initialised: the launch reads only what it wrote itself
 *   out       double [nimg][nbands], every element written.  Per-tile partial sums are f32, their fold is in double and in a fixed
 *             order; no atomics: the same input gives the same bits.
 * No global state; every launch goes to `stream`. */
int fw_band_stats(int src_kind, const void* src, const unsigned char* clean, const unsigned char* ring, const float* panels_h,
                  const float* panels_w, float* work, double* out, int nimg, int H, int W, int nbands, int power, void* stream);
/* The bands themselves, of maps of ANY size (csrc/fw_spec.hip; net/utils/frequency_decompose.py:5-125 for any (h, w)).  With
 * M_b[u][v] = (ring[u][v] == b) and F_n = the un-normalised DFT2 of map n:
 *   mode 0  band images   out f32 [nbands][nimg][H][W]    = Re IDFT2(M_b F_n), normalised by 1 / (H W)              (inverse=True)
 *        1  masked spectra out f32 [nbands][nimg][H][W][2] = (re, im) of M_b F_n, UN-shifted coordinates; 8-byte aligned (inverse=False)
 *        2  magnitudes    out f32 [nbands][nimg][H][W]    = |M_b F_n| in fftshift-ed coordinates of the two map axes: the bin (u, v) at
 *                         [(u + H / 2) % H][(v + W / 2) % W] (integer H / 2, W / 2: DC at [H / 2][W / 2], odd sides included)
 * src_kind, src, clean, ring, panels_h, panels_w, the ranges of H, W, nbands and nimg: exactly as for fw_band_stats; mode outside
 * 0..2, like any other argument out of range, is the argument error and nothing is launched.  The ring may be ANY table: it need not
 * be point-symmetric (mode 0 weights each bin of the half spectrum with the mean of its own and its mirror bin's membership, which is
 * exact for the real part) nor a partition (a bin >= nbands is in no band).
 *   work      f32, nimg * Hp * Wh * 4 floats in modes 1 and 2, nimg * Hp * Wh * (4 + 2 * min(nbands, 4)) floats in mode 0 (Hp, Wh as
 *             for fw_band_stats: T^t and the half spectrum F^t, re and im, and in mode 0 the column-inverted bands G of up to 4 bands
 *             at a time); 16-byte aligned; need not be initialised: the launch reads only what it wrote itself
 *   out       EVERY element is written, those of a band without bins with 0.
 * f32 products and sums on the matrix cores as in fw_band_stats; no atomics: the same input gives the same bits.  No global state;
 * every launch goes to `stream`. */
int fw_band_split(int src_kind, const void* src, const unsigned char* clean, const unsigned char* ring, const float* panels_h,
                  const float* panels_w, float* work, float* out, int nimg, int H, int W, int nbands, int mode, void* stream);

/* ---- encoder contrastive head: BatchNorm2d + LeakyReLU(0.1) + GAP (encoder_Uformer.py:945-951,978-984) -- */
int fw_bn_lrelu_gap_fwd(int dtype, const void* fea, const float* gamma, const float* beta, float* rmean, float* rvar,
                        long long* nbt, float* part, float* saved, float* gap, int B, int ED, int P, int training, float eps,
                        float momentum, float slope, void* stream);
int fw_bn_lrelu_gap_bwd(int dtype, const void* fea, const float* gamma, const float* beta, const float* saved, const float* dgap,
                        float* part2, void* dfea, float* dgamma, float* dbeta, int B, int ED, int P, float slope, void* stream);

/* ---- MoCo logits / enqueue (net/utils/moco.py:127-164, 52-66) ---------------------------------------- */
int fw_moco_logits(const float* q, const float* k, const float* queue, float* logits, float* khat, int L, int B, int ED, int K,
                   float invT, void* stream);
int fw_moco_logits_bwd(const float* q, const float* khat, const float* queue, const float* dlogits, float* dq, int L, int B,
                       int ED, int K, float invT, void* stream);
int fw_moco_enqueue(float* queue, const float* khat, long long* ptr, int L, int B, int ED, int K, void* stream);

/* ---- learned-frequency-selection lambda heads of all decoder blocks (decoder_Uformer.py:178-193,279-284) --
 * fw_lfs_lambda_bwd ADDS into the tensors gtab names, each word once with a plain read-modify-write by the workgroup that owns its
 * (block, band): two entries of gtab must not name the same memory, and nothing else may write it while the launch runs.  dxbar,
 * shared by all blocks, is added with atomics. */
int fw_lfs_xbar(const float* inter, float* xbar, float* stats, int nb1, int B, int NT, int C, float eps, void* stream);
int fw_lfs_xbar_bwd(const float* inter, const float* stats, const float* dxbar, float* dinter, int nb1, int B, int NT, int C,
                    void* stream);
int fw_lfs_lambda(const float* xbar, const unsigned long long* ptab, const int* heads, const long long* coef_off, float* coef,
                  float* save, int nblk, int B, int C, int nb1, void* stream);
int fw_lfs_lambda_bwd(const float* xbar, const unsigned long long* ptab, const unsigned long long* gtab, const int* heads,
                      const long long* coef_off, const float* dcoef, const float* save, float* dxbar, int nblk, int B, int C,
                      int nb1, void* stream);

/* ---- convolutional plug-ins of the seam: ResNetEncoder (net/encoder_ResNet.py:4-47), DGRN (net/decoder_DGRN.py:9-158) ----
 * fw_conv3x3: nn.Conv2d k3 p1 (taps 0x1ff) or k1 p0 (taps 0x010: weights at the centre tap of the same panel), stride 1 | 2, as
 * an implicit GEMM on MFMA (decoder_DGRN.py:5-6 default_conv, :37-47 SFT 1x1 convs; encoder_ResNet.py:8,11,15 ResBlock convs;
 * deform_conv.py:31-36 conv_offset_mask on cat[x, inter] = channels [0, cin1) from x, [cin1, cin) from x2).  x, x2, res: T
 * [B*H*W][ld] token-major; w: T [roundup(cout, 16)][9 * cin], element (co, tap, ci); out: T or f32 [B*Ho*Wo][ldo];
 * epilogue: + bias[co], act 1 = LeakyReLU(slope), + res.  With a flipped, transposed panel it is the input gradient of a
 * stride-1 convolution. */
int fw_conv3x3(int dtype, const void* x, long ldx, const void* x2, long ldx2, int cin, int cin1, const void* w, const float* bias,
               void* out, long ldo, int out_f32, const void* res, long ldr, int cout, int B, int H, int W, int stride, int taps,
               int act, float slope, void* stream);
/* explicit [tokens][9 * C] operand of a 3x3 p1 convolution (weight gradients; input gradients of stride-2 convolutions) */
int fw_im2col3(int dtype, const void* x, long ldx, void* col, int B, int H, int W, int C, int stride, void* stream);
int fw_col2im3(int dtype, const void* dcol, void* dx, long lddx, int B, int H, int W, int C, int stride, void* stream);
/* DCNv2, net/utils/deform_conv.py:56-67 (the reference's call into mmcv is commented out and the function asserts: parity
 * unpinned).  om: f32 [B*H*W][32] raw conv_offset_mask output, channels 2k / 2k+1 = (dy, dx) of tap k, 18 + k = mask logit.
 * fw_dcn_im2col: col[p][k * C + c] = sigmoid(mask_k) * bilinear(x[:, c], p + p_k + offset_k) -- the operand of a plain GEMM with
 * the [Cout][9 * Cin] weight.  fw_dcn_bwd: dx (f32, accumulated: pre-zero) and dom from d(col). */
int fw_dcn_im2col(int dtype, const void* x, long ldx, const float* om, void* col, int B, int H, int W, int C, void* stream);
int fw_dcn_bwd(int dtype, const void* dcol, const void* x, long ldx, const float* om, float* dx, long lddx, float* dom, int B, int H,
               int W, int C, void* stream);
/* nn.BatchNorm2d (+ residual add + LeakyReLU) on a token-major map, encoder_ResNet.py:9-10,12,16,20.  sums: f32 [2][C] zeroed
 * scratch; mr: f32 [2][C] (mean, rstd) out.  Backward: on return sums[0] = d(beta), sums[1] = d(gamma); dres = dy * lrelu'(y). */
int fw_bn_cl_fwd(int dtype, const void* x, long ldx, const float* gamma, const float* beta, float* rmean, float* rvar, long long* nbt,
                 float* sums, float* mr, const void* res, long ldr, void* y, long ldy, long rows, int C, int training, float eps,
                 float momentum, float slope, void* stream);
int fw_bn_cl_bwd(int dtype, const void* dy, long ldd, const void* y, long ldy, const void* x, long ldx, const float* mr,
                 const float* gamma, float* sums, void* dx, long lddx, void* dres, long lddr, long rows, int C, int training,
                 float slope, void* stream);
/* nn.LeakyReLU on T maps (decoder_DGRN.py:40,45 inside the SFT MLPs) and its backward from the OUTPUT's sign */
int fw_lrelu_t(int dtype, const void* x, long ldx, void* y, long ldy, long rows, int C, float slope, void* stream);
int fw_lrelu_t_bwd(int dtype, const void* dy, long ldd, const void* y, long ldy, void* dx, long lddx, long rows, int C, float slope,
                   void* stream);
/* DGM + the LeakyReLU DGB applies to it (decoder_DGRN.py:22-32,79,81): out = lrelu(x + dcn + x * gamma + beta); backward:
 * dz = dout * lrelu'(out) (= d dcn = d beta), dx = dz (1 + gamma), dgamma = dz x.  Contiguous T tensors of n elements. */
int fw_dgm_fwd(int dtype, const void* x, const void* dcn, const void* gamma, const void* beta, void* out, long n, float slope,
               void* stream);
int fw_dgm_bwd(int dtype, const void* dout, const void* out, const void* x, const void* gamma, void* dx, void* dz, void* dgamma,
               long n, float slope, void* stream);
/* nn.AdaptiveAvgPool2d(1) on a token-major map (encoder_ResNet.py:33): [B * P][C] T -> f32 [B][C] */
int fw_gap_cl(int dtype, const void* x, long ldx, float* out, int B, int P, int C, void* stream);
int fw_gap_cl_bwd(int dtype, const float* dgap, void* dx, long lddx, int B, int P, int C, void* stream);
/* image planes f32 [B][Ci][H*W] <-> token-major T [B*H*W][ld] (channels Ci .. Cp-1 zero-filled) */
int fw_nchw_to_tokens(int dtype, const float* img, void* tok, long ld, int B, int Ci, int HW, int Cp, void* stream);
int fw_tokens_to_nchw(int dtype, const void* tok, long ld, float* img, int B, int Ci, int HW, void* stream);

/* ---- ViT encoder plug-in (net/encoder_ViT.py:17-203) --------------------------------------------------------------------
 * The transformer body runs on fw_layernorm_*, fw_gemm and fw_attn_* (head_dim 64, one 64-token window per image, zero
 * bias table: encoder_ViT.py:76-98 without the band re-weighting); these cover the rest:
 * fw_add_bcast: x += self.pos_embedding[:, :n] (encoder_ViT.py:187);  out[i] = x[i] + p[i % period].
 * fw_bn_planes_*: self.norm (BatchNorm2d + LeakyReLU 0.1) and self.avg on the [B][ED][P] planes of `inter` (:170-173,194-199); both
 *   the normalised map (returned as `inter`) and the pooled vector are materialised, the backward takes gradients of both.
 * fw_small_linear_*: the encoder_dim x encoder_dim MLP head (:175-179; encoder_dim = 3 by default), y = lrelu(x W^T + b, slope). */
int fw_add_bcast(const float* x, const float* p, float* out, long n, long period, void* stream);
int fw_bn_planes_fwd(int dtype, const void* fea, const float* gamma, const float* beta, float* rmean, float* rvar, long long* nbt, float* mr,
                     float* inter, float* gap, int B, int ED, int P, int training, float eps, float momentum, float slope, void* stream);
int fw_bn_planes_bwd(int dtype, const void* fea, const float* inter, const float* gamma, const float* mr, const float* dinter,
                     const float* dgap, void* dfea, float* dgamma, float* dbeta, int B, int ED, int P, int training, float slope,
                     void* stream);
int fw_small_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int N, int K, float slope, void* stream);
int fw_small_linear_bwd(const float* dy, const float* y, const float* x, const float* w, float* dx, float* dw, float* db, int M, int N,
                        int K, float slope, void* stream);

/* ---- ViT global attention (net/encoder_ViT.py:76-98 `Attention.forward`; BASELINE configs[4]: N = 256 tokens at 256x256) -----
 * q | k | v: T [B*N][ld], head h at column h * 64 (head_dim 64); N in {64, 256}, or any other multiple of 64 from 128 to 1024
 * (576 at 384x384, 1024 at 512x512; lamb at 576 and 1024 only, NULL elsewhere).  out: T [B*N][heads*64]; lse: f32 [B][heads][N].
 * attn = softmax(q k^T scale) [+ sum_i lamb[i] band_i(attn)] -> dropout(p) -> attn v, one workgroup per (image, head, 64 queries),
 * the 64 x N score block in registers at N in {64, 256}; at the other N the key tiles stream past with an online softmax (same lse,
 * same mask indices).  Dropout (encoder_ViT.py:67,94): counter-based mask of (seed[0], site, flat index of the
 * [B][heads][N][N] map), re-derived by the backward pass; drop_p = 0 or eval: off.  lamb (optional, N = 64 only -- the reference's
 * masks are dim_head x dim_head, encoder_ViT.py:56,60): f32 [nb][lamb_batch (1 | B)][heads] of encoder_ViT.py:62-66,85-92, evaluated
 * as a 64x64 2-D DFT on the f32 MFMA; bandidx: u8 [64][64] band of every un-shifted spectrum bin; panels: f32 cos[64][64], sin[64][64].
 * N in {256, 576, 1024} with lamb: only the 'DC' decomposition on the N x N grid (encoder_ViT.py:59-60 'frequency_decompose_dc' with
 * masks sized by the map): nb = 2, bandidx = panels = NULL; band 0 is the mean of the map, 1 / N for softmax rows, so the kernel
 * evaluates attn' = (1 + lamb[1]) attn + (lamb[0] - lamb[1]) / N without a transform (at 576 / 1024 the streaming forward keeps a
 * second, unrescaled accumulator for the constant term); `<n>_bands` is fw_gattn_bands_fwd / bwd at N = 256 / 576 /
 * 1024, which require the tables.  Every other lamb / N combination (any lamb at N not in {64, 256, 576, 1024}
 * included) and every other N is an argument error. */
int fw_gattn_fwd(int dtype, const void* q, const void* k, const void* v, long ld, void* out, long ldo, float* lse, int B, int heads, int N,
                 float scale, const void* seed, int site, float drop_p, const float* lamb, int nb, int lamb_batch, const void* bandidx,
                 const float* panels, void* stream);
/* Same domain as fw_gattn_fwd.  dq, dk, dv: T, same layout as q / k / v (row stride ldd); dvec: f32 [B][heads][N] scratch
 * (rowsum(dO . O); unused with lamb at N = 64, required with lamb at N = 256 / 576 / 1024, where it receives rowsum(P . dP));
 * dlamb: accumulated (atomics), same layout as lamb. */
int fw_gattn_bwd(int dtype, const void* q, const void* k, const void* v, long ld, const void* o, long ldo, const void* dout, long lddo,
                 const float* lse, float* dvec, void* dq, void* dk, void* dv, long ldd, int B, int heads, int N, float scale,
                 const void* seed, int site, float drop_p, const float* lamb, float* dlamb, int nb, int lamb_batch, const void* bandidx,
                 const float* panels, void* stream);
/* The same attention with `<n>_bands` masks sized by the map, N in {256, 576, 1024} (256x256 / 384x384 / 512x512 inputs) -- any other
 * N is an argument error; encoder_ViT.py:55-56,85-92 with FrequencyDecompose('frequency_decompose', 1/nb, N, N) in place of the
 * dim_head-sized masks.  bandidx: u8 [N][N] (symmetric); panels: f32 [2][N][N], cos then sin of 2 pi u i / N.  The map leaves the
 * workgroup: a probabilities kernel, the passes of a batched N x N 2-D DFT on the f32 MFMA (attn += Re IDFT2(W . DFT2(attn))), and an
 * apply kernel (Dropout, attn v).
 *   N = 256: row / column / output passes through LDS.
 *   N = 576 / 1024: four LDS-free 64x64-tile passes (row, column with the lamb weights, inverse column, output) after a probabilities
 *     kernel that walks the key tiles twice (online lse, then attn = exp(s scale - lse) as f32); B * heads <= 65535.
 * amap: f32 [B*heads][N][N], receives attn' = attn + filter(attn) (before Dropout) and is what the backward pass needs.
 * work: scratch of W * B*heads * N * N floats, W planes per map:   forward  W = 2 at N = 256, 4 at N = 576 / 1024
 *                                                                  backward W = 4 at N = 256, 6 at N = 576 / 1024
 *   (the transform planes, and in the backward pass the spectrum of the probabilities that lamb is differentiated against). */
int fw_gattn_bands_fwd(int dtype, const void* q, const void* k, const void* v, long ld, void* out, long ldo, float* lse, int B, int heads,
                       int N, float scale, const void* seed, int site, float drop_p, const float* lamb, int nb, int lamb_batch,
                       const void* bandidx, const float* panels, float* amap, float* work, void* stream);
/* amap: as the forward pass left it; pmap, gmap: f32 [B*heads][N][N] scratch (the probabilities rebuilt from lse; the map gradient,
 * filtered in place: the filter is self-adjoint); work: as above; dvec: f32 [B][heads][N] scratch; dlamb accumulated: sum over band
 * of Re(X_P conj(X_G)) / N^2, one atomic per workgroup and band. */
int fw_gattn_bands_bwd(int dtype, const void* q, const void* k, const void* v, long ld, const void* dout, long lddo, const float* lse,
                       float* dvec, void* dq, void* dk, void* dv, long ldd, int B, int heads, int N, float scale, const void* seed, int site,
                       float drop_p, const float* lamb, float* dlamb, int nb, int lamb_batch, const void* bandidx, const float* panels,
                       const float* amap, float* pmap, float* gmap, float* work, void* stream);
/* nn.Dropout call sites of the ViT (encoder_ViT.py:31,33,73,158,189) with the same counter-based masks.  mode 0: y = drop(x) (f32);
 * 1: y = res + drop(x) (f32); 2: y = drop(gelu(x)) (T); 3: y = drop(x) * gelu'(aux) (T, backward of 2); 4: y = drop(x + aux[i % period])
 * (f32: pos_embedding add + emb dropout, encoder_ViT.py:187-189).  n = elements of the contiguous tensor; p = 0: identity masks. */
int fw_dropout(int mode, int dtype, const void* x, const void* aux, const float* res, void* y, long n, long period, const void* seed, int site,
               float p, void* stream);
/* seed[0] += 1 (u32 in device memory): once per training step, inside the captured graph */
int fw_rng_tick(void* seed, void* stream);

/* ---- callers either side of the model -----------------------------------------------------------------------
 * fw_train_batch: one launch = one training batch from uint8 images resident in HBM (utils/dataset_utils.py:122-135,
 * utils/image_utils.py:133-182): tab: device int64 [B][4] = {clean u8 [3][H][W], degraded u8 or 0, H, W}; rnd: device int32 [B][6] =
 * non-negative random integers {y1, x1, mode1, y2, x2, mode2} (crop origin = r % (H - S + 1), mode = 1 + r % 7); sigma: f32 [B] noise
 * level used when no degraded image is given: clip(gt + z * sigma, 0, 255) truncated to the uint8 grid, z = counter-based N(0, 1) of
 * (seed[0], site + b, pixel) -- both crops see the SAME noisy image.  Outputs f32 [B][3][S][S] in [0, 1] (ToTensor): degraded crop 1 / 2,
 * clean crop 1 / 2. */
int fw_train_batch(const void* tab, const int* rnd, const float* sigma, const void* seed, int site, float* d1, float* d2, float* c1,
                   float* c2, int B, int S, void* stream);
/* fw_train_batch with rain, haze and motion blur synthesised in the launch (stand-ins for the paired sets, fwair/augment.py).  prm: device
 * int32 [B][8] = {code, p1, p2, p3, p4, 0, 0, 0}; code 0: the slot behaves as in fw_train_batch.  ray: device int8 [32][32][2], (dy, dx) =
 * (round(t sin), round(t cos)) of step t at angle pi a / 32; hazet: device uint16 [16][256] = round(65535 exp(-beta_j (1 - 0.9 k / 255))).
 * With g = the clean value of source pixel (c, y, x) of the full H x W image, all in integers:
 *   1 rain {a, L <= 32, density16, S8}: q is a seed iff (h & 0xFFFF) < density16, h = hash32((qy W + qx) ^ key(seed[0], site + b)), of
 *     amplitude A(q) = 128 + ((h >> 16) & 127); m = max over t < L, q = (y, x) - ray[a][t] inside the image and a seed, of A(q) (L - t);
 *     d = min(255, g + m S8 / (256 L)).
 *   2 haze {j, A8}: k = 255 y / (H - 1), T = hazet[j][k], d = (g T + A8 (65535 - T) + 32767) / 65535.
 *   3 motion blur {a, n odd <= 25}: d = (2 sum + n) / (2 n), sum over s = -(n-1)/2 .. (n-1)/2 of the clean value at (y, x) + sign(s)
 *     ray[a][|s|], clamped at the image border.
 * Both crops of a slot cut the same degraded image; the rain layer is new in every slot and call (site).  Parameters outside the tables'
 * extent are clamped. */
int fw_train_batch_synth(const void* tab, const int* rnd, const float* sigma, const int* prm, const void* ray, const void* hazet,
                         const void* seed, int site, float* d1, float* d2, float* c1, float* c2, int B, int S, void* stream);
/* The degraded image of ONE sample as uint8 [3][H][W], by the same per-pixel code (prm: one record of code 1..3; key(seed[0], site)). */
int fw_synth_image(const void* clean, const int* prm, const void* ray, const void* hazet, const void* seed, int site, void* out, int H,
                   int W, void* stream);
/* test.py:47-57: tiles[t = a * nx + b][c][i][j] = img[c][ys[a] + i][xs[b] + j]  (ys / xs: device int32 tile origins) */
int fw_tile_gather(const float* img, const int* ys, const int* xs, float* tiles, int C, int H, int W, int ny, int nx, int T, void* stream);
/* test.py:61-71 with the RESTORED tiles: out[c][y][x] = mean of the tiles covering (y, x) */
int fw_tile_blend(const float* tiles, const int* ys, const int* xs, float* out, int C, int H, int W, int ny, int nx, int T, void* stream);
/* utils/val_utils.py:50-66 (skimage structural_similarity defaults: 7x7 uniform window, K1 .01, K2 .03, sample covariance, 3-pixel
 * border cropped, inputs clipped to [0, 1]): out[i] += sum of the SSIM map of image i over channels and interior pixels. */
int fw_ssim7(const float* a, const float* b, float* out, int n, int C, int H, int W, void* stream);
/* The same three steps for a CHUNK of test images of different sizes, one launch each, driven by tables in device memory
 * (fwair/evaluate.py EvalEngine).  itab: int64 [I][4] = {clean u8 [3][H][W] or 0, degraded u8 or 0, H, W}; ttab: int32 [N][4] =
 * {image, y0, x0, 0}, the tiles of the chunk, image by image, rows major; gtab: int64 [I][4] = {offset of the image in the packed
 * buffer (elements), its first tile in the chunk, ny, nx}.  T % 4 == 0.
 * fw_eval_gather (test.py:47-57 on utils/dataset_utils.py:174-185): tiles f32 [N][3][T][T] = the degraded image / 255 where one is
 * given; otherwise the clean image with the test set's noise synthesised in the kernel, floor(clip(g + z * sigma[image], 0, 255)) / 255,
 * z = the counter-based N(0, 1) of fw_train_batch at (seed[0], site + image, flat CHW pixel index of the full image): overlapping
 * tiles see the same noisy image, which is never stored.  sigma[image] = 0: the clean image itself. */
int fw_eval_gather(const void* itab, const int* ttab, const float* sigma, const void* seed, int site, float* tiles, int N, int T,
                   void* stream);
/* test.py:61-71 with the RESTORED tiles for images i0 .. i0 + nimg - 1 (ttab: the chunk's tiles, ntiles of them; rest: f32
 * [ntiles][3][T][T]): packed[gtab offset ..] = the overlap average, f32 [3][H][W] per image; sse[image] += sum of (clip(restored) -
 * clean / 255)^2 over the image (utils/val_utils.py:52-63; skipped without a clean image), one atomic per workgroup; u8out (or 0):
 * (uint8) clip(restored * 255, 0, 255) at the same offsets (utils/image_io.py:383). */
int fw_eval_blend(const void* itab, const void* gtab, const int* ttab, const float* rest, float* packed, void* u8out, float* sse,
                  int i0, int nimg, int ntiles, int T, void* stream);
/* utils/val_utils.py:64 as fw_ssim7 computes it, between the packed restored images and the clean uint8 images of the tables:
 * out[image] += sum of the SSIM map over channels and interior pixels, for images i0 .. i0 + nimg - 1. */
int fw_eval_ssim7(const void* itab, const void* gtab, const float* packed, float* out, int i0, int nimg, void* stream);
/* fw_eval_gather / fw_eval_blend for images of any size, overlapping tiles and the x8 self-ensemble (fwair/evaluate.py plan_tiles_ex).
 * itab as above; ttab: int32 [N][4] = {image, y0, x0, mode}, where [y0, y0 + T) x [x0, x0 + T) may leave the image and mode (taken & 7)
 * is one of fw_train_batch's flips / rotations (utils/image_utils.py:133-175) with 0 = none; gtab: int64 [I][8] = {offset of the image in
 * the packed buffer (elements), its first tile in the chunk, ny, nx, stride, nmodes (1 or 8), 0, 0}: tile (a, b, m) of the image is row
 * first + (a nx + b) nmodes + m of ttab.  (fw_eval_ssim7 takes the first four columns as a table of its own.)
 * fw_restore_gather: tiles[t][c][oy][ox] = source[c][R(y0 + py, H)][R(x0 + px, W)] / 255, (py, px) = the preimage of (oy, ox) under mode:
 * k = mode >> 1, ii = (mode & 1) ? T - 1 - oy : oy, jj = ox; k = 0: (ii, jj), 1: (jj, T - 1 - ii), 2: (T - 1 - ii, T - 1 - jj),
 * 3: (T - 1 - jj, ii).  R = whole-sample reflection continued periodically: R(y, 1) = 0, otherwise p = 2 n - 2, m = ((y mod p) + p) mod p,
 * R = m < n ? m : p - m (np.pad 'reflect' for every pad width), so no origin reads outside the image.  The source is the degraded image
 * or the clean one with fw_eval_gather's noise, whose counter is the flat CHW index of the SOURCE pixel in the unpadded image:
 * reflected copies, overlapping tiles and the eight turns see one noisy image. */
int fw_restore_gather(const void* itab, const int* ttab, const float* sigma, const void* seed, int site, float* tiles, int N, int T,
                      void* stream);
/* packed / u8out / sse as fw_eval_blend writes them, with out[c][y][x] = sum(w v) / sum(w) over the tiles (a, b, m) whose footprint in
 * the image holds (y, x), in ascending tile order (at most 3 x 3 x 8 terms when the overlap is at most T / 2): v = rest[t][c][oy][ox] at
 * the image of (y - y0, x - x0) under the tile's mode (the turn undone), w = w1(y - y0) w1(x - x0), w1(i) = (float)min(i + 1, T - i, ramp) /
 * (float)ramp (symmetric, so the same in every mode; the quotient and the product rounded once each).  ramp = 1: fw_eval_blend's plain
 * mean.  1 <= ramp <= T / 2 or ramp == 1.  Candidates per axis: the regular tiles a stride <= y < a stride + T with a <= ny - 2, and
 * tile ny - 1.  Gather form, no atomics on pixels. */
int fw_restore_blend(const void* itab, const void* gtab, const int* ttab, const float* rest, float* packed, void* u8out, float* sse,
                     int i0, int nimg, int ntiles, int T, int ramp, void* stream);

/* ---- fused LeFF forward (net/utils/leff.py:92-117) for the high-resolution stages, bf16 operands ----------------------------
 * y = res + rowscale * linear2(GELU(dwconv3x3(GELU(linear1(xn))))) in one kernel per 8 x 16 pixel patch: the hidden tensor is
 * produced and consumed on chip (7 chunks of 4C/7 channels); h1, g1, h2, g2 (bf16 [T][4C]) are WRITTEN for the unfused backward
 * kernels, never re-read.  w1p: bf16 [4C][roundup(C, 32)] zero-padded; w2p: bf16 [roundup(C, 16) + 1][4C] zero rows;
 * wd: f32 [9][4C] tap-major.  C in {28, 56, 112}, H % 8 == 0, W % 16 == 0. */
int fw_leff_fwd(const void* xn, long ldx, const void* w1p, const float* b1, const float* wd, const float* bd, const void* w2p,
                const float* b2, const float* res, long ldr, const float* rowscale, int rows_per_scale, float* y, long ldy, void* h1,
                void* g1, void* h2, void* g2, long ldh, int B, int H, int W, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
