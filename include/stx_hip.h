/* stx_hip.h -- C-ABI of libstx_hip.so: the MI355X (gfx950) cost-volume hot path of
 * xxxupeng/stereo_toolbox (PSMNet / GwcNet / ACVNet).
 *
 * The reference is 100 % Python/PyTorch and has no FFI of its own; each entry point below replaces a
 * *torch-op sequence* of the reference (file:line relative to /root/reference/stereo_toolbox).  This
 * is the boundary a maintainer binds (ctypes stub in INTEGRATION.md; stereo_toolbox_amd/_capi.py is
 * the binding this repo ships).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to dense fp32 data unless noted; `stream` is a hipStream_t
 *     (NULL = default stream); calls are asynchronous on that stream, never synchronise, never
 *     allocate; all scratch memory is passed in by the caller;
 *   - 2-D features are NCHW [B][C][H][W]; 3-D activations are channels-last [B][D][H][W][C];
 *   - return value 0 = OK; 1 = invalid argument; 2 = launch failure; stx_last_error() gives the
 *     message of the last failure on the calling thread;
 *   - re-entrant: no mutable state beyond the tuning switches below, safe from several host threads / one process
 *     per GPU.
 */
#ifndef STX_HIP_H
#define STX_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

const char* stx_last_error(void);
const char* stx_build_info(void);
/* Tuning / A-B switches (names = their environment variables, e.g. "STX_MARCH_BS"; list and defaults: StxTune in
 * csrc/stx_common.h, and STX_DA_GRID in csrc/stx_runtime.hip).  The environment is read ONCE, when the library is loaded; stx_set_tuning changes a switch for the
 * calls that follow in this process (tests, tools/kernel_bench.py).  None changes a result beyond fp32 rounding.
 * stx_get_tuning: value, or -1 for an unknown name;  stx_set_tuning: 0, or 1 for an unknown name. */
int stx_get_tuning(const char* name);
int stx_set_tuning(const char* name, int value);

/* ---- cost-volume builders ------------------------------------------------------------------
 * build_gwc_volume / groupwise_correlation  models/GwcNet/submodule.py:44-63 (dup ACVNet/submodule.py:209-238)
 * build_concat_volume                       models/GwcNet/submodule.py:30-41, PSMNet/stackhourglass.py:111-120
 *                                           (mask_left=1), ACVNet/submodule.py:180-191 (mask_left=0)
 * torch.cat((gwc, concat), 1)               models/GwcNet/gwcnet.py:180 (fused)
 * softmax(att, dim=2) * concat_volume       models/ACVNet/acv.py:196 (`scale` = softmax probabilities [B][D][H][W], or NULL)
 * vol: [B][D][H][W][G + 2*Cc].  Lg/Rg: [B][Cg][H][W] (NULL when G == 0); Lc/Rc: [B][Cc][H][W] (NULL when Cc == 0).
 * Requires Cg % G == 0 (reference assert submodule.py:46), Cg/G in {4,8,12,16} (and 20 / 28 with 4..16 groups: FoundationStereo's
 * 160 / 224-channel maps in 8 groups), G % 4 == 0, Cc % 4 == 0. */
int stx_cost_volume_fwd(const float* Lg, const float* Rg, int Cg, int G, const float* Lc, const float* Rc, int Cc,
                        const float* scale, float* vol, int B, int H, int W, int D, int mask_left, void* stream);
/* Per-pixel, per-group L2 normalisation of an NCHW map, the pre-pass of FoundationStereo's normalised group-wise correlation
 * (models/FoundationStereo/submodule.py:388-397: F.normalize(fea.float(), dim=2) on [B,G,C/G,H,W], eps 1e-12, group SUM):
 * y[b][c][p] = out_scale * x[b][c][p] / max(||x[b][group of c][p]||_2, 1e-12).  The normalised volume (:399-413) is
 * stx_cost_volume_fwd of the two normalised maps with out_scale = C/G on the left one (group mean x C/G = group sum).
 * x, y, gy, gx: [B][C][HW]; C % G == 0 (reference assert :390). */
int stx_group_normalize_fwd(const float* x, float* y, int B, int C, int G, int HW, float out_scale, void* stream);
int stx_group_normalize_bwd(const float* x, const float* gy, float* gx, int B, int C, int G, int HW, float out_scale, void* stream);
/* autograd backward of the above (no `scale`): gvol [B][D][H][W][G+2Cc] -> gLg,gRg [B][Cg][H][W], gLc,gRc [B][Cc][H][W] */
int stx_cost_volume_bwd(const float* gvol, const float* Lg, const float* Rg, int Cg, int G, int Cc, float* gLg,
                        float* gRg, float* gLc, float* gRc, int B, int H, int W, int D, int mask_left, void* stream);

/* ---- regression head and disparity estimators ---------------------------------------------------
 * F.upsample(trilinear) -> squeeze -> F.softmax(dim=1) -> disparity_regression, fused:
 *   models/GwcNet/gwcnet.py:197-224, models/PSMNet/stackhourglass.py:139-153, models/ACVNet/acv.py:206-251.
 * cost [B][Dc][Hc][Wc] -> disp [B][H][W]; stats [B][H][W][2] (per-pixel max and sum-exp, kept for backward; may be NULL). */
int stx_head_fwd(const float* cost, float* disp, float* stats, int B, int Dc, int Hc, int Wc, int D, int H, int W,
                 void* stream);
/* backward (deterministic, two passes); workspace: stx_head_bwd_workspace_floats(B, Dc, H, W) floats */
long long stx_head_bwd_workspace_floats(int B, int Dc, int H, int W);
int stx_head_bwd(const float* gdisp, const float* cost, const float* disp, const float* stats, float* gcost,
                 float* workspace, int B, int Dc, int Hc, int Wc, int D, int H, int W, void* stream);
/* the same two with an explicit interpolation rule: align_corners != 0 is F.upsample(..., align_corners=True), the
 * head of the PCWNet / CFNet family (models/PCWNet/pcwnet.py:446-470); align_corners == 0 equals the entries above */
int stx_head_fwd2(const float* cost, float* disp, float* stats, int B, int Dc, int Hc, int Wc, int D, int H, int W,
                  int align_corners, void* stream);
int stx_head_bwd2(const float* gdisp, const float* cost, const float* disp, const float* stats, float* gcost,
                  float* workspace, int B, int Dc, int Hc, int Wc, int D, int H, int W, int align_corners, void* stream);
/* disparity_regression (GwcNet/submodule.py:23-27), disparityregression (PSMNet/submodule.py:46-54),
 * softargmax_disparity_estimator (disparity_estimators/__init__.py:7-10): out[b][hw] = sum_d d * x[b][d][hw] */
int stx_softargmax_fwd(const float* x, float* out, int B, int D, int HW, void* stream);
/* argmax_disparity_estimator (disparity_estimators/__init__.py:13-15): out int64 [B][HW], first maximum */
int stx_argmax_fwd(const float* x, long long* out, int B, int D, int HW, void* stream);
/* unimodal_disparity_estimator (disparity_estimators/unimodal_disparity_estimator.py:4-25) and
 * dominant_modal_disparity_estimator (disparity_estimators/dominant_modal_disparity_estimator.py:35-54):
 * x [B][D][HW] probability volume (D = maxdisp) -> out [B][HW], the re-normalised expectation of d over the mode that
 * contains the arg-max / over the heavier of the two main modes of the 5-tap-blurred volume. 0/0 -> NaN as in the
 * reference. */
int stx_unimodal_fwd(const float* x, float* out, int B, int D, int HW, void* stream);
int stx_dominant_modal_fwd(const float* x, float* out, int B, int D, int HW, void* stream);
/* The same two estimators with their backward pass (kind 0: unimodal, 1: dominant-modal).  The reference functions are
 * differentiable w.r.t. x inside the mode mask, which is a constant of the graph (`x * mask.data`,
 * unimodal_disparity_estimator.py:20; boolean masks, dominant_modal_disparity_estimator.py:45-49; twin logic in
 * loss_functions/split_mode.py:9-35): d out / d x_k = m_k (k - out) / S.  stx_modal_fwd optionally writes
 * aux [B][5][HW] = (lo, hi, xlo, xhi, S): support [lo, hi] minus [xlo, xhi] and its probability mass S;
 * stx_modal_bwd turns g [B][HW], out and aux into gx [B][D][HW] (zero outside the support). */
int stx_modal_fwd(const float* x, float* out, float* aux, int B, int D, int HW, int kind, void* stream);
int stx_modal_bwd(const float* g, const float* out, const float* aux, float* gx, int B, int D, int HW, void* stream);
/* split_mode(x, maxdisp) -> (mode, mask)  (loss_functions/split_mode.py:9-35): the modal estimators' support mask of
 * the RAW volume x [B][D][HW] (arg-max, edges of its mode, symmetrised when the arg-max sits >= 3 bins off centre):
 * mask [B][D][HW] bytes (0 / 1 = the storage of a torch.bool tensor), mode = x * mask (fp32, same shape). */
int stx_split_mode(const float* x, float* mode, unsigned char* mask, int B, int D, int HW, void* stream);
/* F.softmax over the disparity axis of [B][D][HW] (ACVNet attention weights, acv.py:196) */
int stx_softmax_d_fwd(const float* x, float* y, int B, int D, int HW, void* stream);

/* ---- Conv3d / ConvTranspose3d aggregation (fp32 MFMA implicit GEMM) ---------------------------------
 * nn.Conv3d(k=3,p=1,s=1|2, bias=False), nn.Conv3d(k=1), nn.ConvTranspose3d(k=3,s=2,p=1,op=1, bias=False) of
 * convbn_3d / hourglass / dres / classif: models/GwcNet/gwcnet.py:68-153, models/GwcNet/submodule.py:17-20,
 * models/PSMNet/stackhourglass.py:10-84, models/ACVNet/acv.py:56-144.
 * Weights are first re-laid-out on the device into MFMA operand order (w: torch layout [A][B][T], T = k^3):
 *   mode 0: conv forward (w = [Cout][Cin][T]) and ConvTranspose dgrad;  1: stride-1 conv dgrad;
 *   mode 2: ConvTranspose forward (w = [Cin][Cout][T]) and stride-2 conv dgrad. */
long long stx_conv3d_packed_floats(int K, int N, int T);
int stx_conv3d_pack_weight(const float* w, float* wp, int A, int B, int T, int mode, void* stream);
/* out = act(conv(x) * scale[c] + bias[c] + residual); `relu` is the activation code: 0 none, 1 ReLU, 2 Mish, 3 LeakyReLU(0.01)
 * (x * tanh(softplus(x)), models/PCWNet/submodule.py:11-18); scale/bias/residual may be NULL; if `stats` != NULL the
 * per-workgroup (sum, sum of squares) of the RAW conv output are written to stats[rows][2][Cout] for train-mode
 * BatchNorm: rows = stx_conv3d_fwd_stat_rows(same shape arguments) -- every one of these rows is written, nothing beyond
 * them is touched (no zero-fill pass: hand exactly `rows` rows to stx_bn_finalize).  Cin % 8 == 0, Cout <= 128.
 * stx_conv3d_fwd_blocks(Do,Ho,Wo) * B is an upper bound of `rows` for any channel configuration. */
int stx_conv3d_fwd_blocks(int Do, int Ho, int Wo);
long long stx_conv3d_fwd_stat_rows(int B, int Di, int Hi, int Wi, int Cin, int Cout, int ks, int stride);
int stx_conv3d_fwd(const float* x, const float* wp, float* out, const float* scale, const float* bias,
                   const float* residual, float* stats, int B, int Di, int Hi, int Wi, int Cin, int Cout, int ks,
                   int stride, int relu, void* stream);
int stx_deconv3d_fwd_blocks(int Di, int Hi, int Wi);
int stx_deconv3d_fwd(const float* x, const float* wp, float* out, const float* scale, const float* bias,
                     const float* residual, float* stats, int B, int Di, int Hi, int Wi, int Cin, int Cout, int Do,
                     int Ho, int Wo, int relu, void* stream);
/* weight gradient dW[cc][cf][T] = sum_o fine[S*o+tap-pad][cf] * coarse[o][cc]
 *   conv: fine = layer input, coarse = grad of output;  ConvTranspose: fine = grad of output, coarse = layer input.
 * workspace: stx_conv3d_wgrad_workspace_floats(...) floats. CF % 32 == 0, CC % 32 == 0. */
long long stx_conv3d_wgrad_workspace_floats(int B, int Dc, int Hc, int Wc, int CF, int CC, int ks, int stride);
int stx_conv3d_wgrad(const float* fine, const float* coarse, float* dw, float* workspace, int B, int Df, int Hf, int Wf,
                     int CF, int Dc, int Hc, int Wc, int CC, int ks, int stride, void* stream);

/* The same weight gradient for a 3x3x3 stride-1 `convbn_3d` (+ ReLU) block in training (reference models/GwcNet/submodule.py:17-20
 * under autograd), taking the gradient gy BEHIND the BatchNorm / activation: the gradient of the raw convolution output
 *   dz = gamma invstd (gy' - sum_g / n - xhat sum_gx / n),  gy' = gy masked by the activation (sign of fmaf(z, scale, shift)),
 *   xhat = (z - mean) invstd,  sums = [2][CC] = rows 0 and 1 of stx_bn_bwd_reduce2's sums,  inv_n = 1 / (B D H W),
 * is formed inside the kernel and also written to `dz` (for the data-gradient launch): the stx_bn_bwd_apply2 pass of the block is
 * not needed.  act: 0 none, 1 ReLU.  gamma may be NULL (ones).  Only shapes stx_conv3d_wgrad_bn_supported accepts; workspace as
 * stx_conv3d_wgrad_workspace_floats(B, D, H, W, CF, CC, 3, 1). */
int stx_conv3d_wgrad_bn_supported(int B, int D, int H, int W, int CF, int CC);
int stx_conv3d_wgrad_bn(const float* x, const float* gy, const float* z, const float* scale, const float* shift, const float* mean,
                        const float* invstd, const float* gamma, const float* sums, float inv_n, int act, float* dz, float* dw,
                        float* workspace, int B, int D, int H, int W, int CF, int CC, void* stream);

/* ---- Axial-planar Conv3d (csrc/conv3d_axial.hip) ----------------------------------------------------
 * The two convolutions of FoundationStereo's Conv3dNormActReduced (reference FoundationStereo/submodule.py:89-114): stride 1,
 * "same" zero padding, dense channels-last fp32 [B][D][H][W][C], exact fp32 MFMA (v_mfma_f32_16x16x4_f32).  Kernel shapes
 * (kd,kh,kw): planar (1,3,3) and axial (kd,1,1) with kd odd, 3 <= kd <= 17.  Cin a multiple of 4 up to 192, Cout up to 192
 * (stx_conv3d_axial_supported); wider outputs than one workgroup serves are sliced inside the launcher.
 * Weights are packed on the device from the torch layout w[A][B][T], T = kd*kh*kw (stx_conv3d_axial_packed_floats(K, N, ...)
 * floats for GEMM-K = K input and N output channels):
 *   mode 0: forward (w = [Cout][Cin][T], K = Cin);  mode 1: data gradient (flipped taps, transposed channels: K = Cout, N = Cin).
 * stx_conv3d_axial_fwd: out = act(conv(x) * scale[c] + bias[c] + residual), epilogue contract of stx_conv3d_fwd (activation
 * code 0..3; scale / bias / residual / stats may be NULL); stats[rows][2][Cout] with rows = stx_conv3d_axial_fwd_stat_rows(same
 * shape arguments): every row is written, nothing beyond is touched.  The data gradient is the same call on mode-1 weights with
 * Cin and Cout exchanged.
 * stx_conv3d_axial_wgrad: dw[CC][CF][T] = sum_vox x[vox + t - pad][cf] * gz[vox][cc] (x: layer input, gz: gradient of the raw
 * output; CF and CC multiples of 4); partial sums in `workspace` (stx_conv3d_axial_wgrad_workspace_floats floats), reduced in a
 * fixed order: bitwise reproducible, no atomics.  Unsupported shapes return an error (the *_floats / *_stat_rows queries 0)
 * and launch nothing. */
int stx_conv3d_axial_supported(int Cin, int Cout, int kd, int kh, int kw);
long long stx_conv3d_axial_packed_floats(int K, int N, int kd, int kh, int kw);
int stx_conv3d_axial_pack_weight(const float* w, float* wp, int A, int B, int kd, int kh, int kw, int mode, void* stream);
long long stx_conv3d_axial_fwd_stat_rows(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw);
int stx_conv3d_axial_fwd(const float* x, const float* wp, float* out, const float* scale, const float* bias,
                         const float* residual, float* stats, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh,
                         int kw, int act, void* stream);
long long stx_conv3d_axial_wgrad_workspace_floats(int B, int D, int H, int W, int CF, int CC, int kd, int kh, int kw);
int stx_conv3d_axial_wgrad(const float* x, const float* gz, float* dw, float* workspace, int B, int D, int H, int W, int CF,
                           int CC, int kd, int kh, int kw, void* stream);

/* ---- ConvGRU cell (csrc/convgru.hip) ----------------------------------------------------------------
 * The cell of the iterative families (reference IGEVStereo/update.py:25-40, the same class in RAFTStereo, DEFOMStereo,
 * StereoAnywhere, FoundationStereo): three 3x3 convolutions (padding 1, stride 1, bias) over [h | x..] / [r h | x..] with fused
 * sigmoid / tanh gates, exact fp32 MFMA.  Activations are channels-last fp32 [B][H][W][C].  The K axis of a convolution is a
 * virtual concatenation of up to 4 SOURCES, each given as (device pointer, channels, pixel pitch in floats): pointer 16-byte
 * aligned, channels a multiple of 4, pitch >= channels and a multiple of 4; unused trailing sources are (NULL, 0, 0).  Served
 * (stx_convgru_supported(hidden, nx, cx0, cx1, cx2, kernel)): hidden a multiple of 16 up to 128, 1..3 x sources (the fourth
 * source is h), hidden + sum cx <= 512, kernel 3.
 * stx_convgru_pack_weight: packs one or two (w1 may be NULL) torch weights [A][Bd][3][3], stacked along A, into
 *   stx_convgru_packed_floats(K, N) floats; mode 0: forward (K = Bd, N = A or 2 A); mode 1: data gradient (flipped taps,
 *   transposed channels: K = A or 2 A, N = Bd).
 * stx_convgru_gemm: acc[pix][n] = conv over the source list with packed weights of N output channels, then the epilogue `epi`:
 *   0 raw: out0[pix][out_pitch] = acc (+ add0[pix][add0_pitch]); out0 may be add0 itself (updated in place);
 *   1 zr:  N = 2 split (split = hidden), z | r stacked: out0 = z = sigmoid(acc + bias0 + add0) [pix][hidden],
 *          out1 = r h with r = sigmoid(acc + bias1 + add1), out2 = r (may be NULL);
 *   2 q:   N = split: q = tanh(acc + bias0 + add0), out0 = h' = (1 - z) h + z q, out1 = q (may be NULL).
 *   bias / add pointers may be NULL (zero); h [pix][h_pitch] is the state at the centre pixel; outputs never alias h.
 * stx_convgru_gate_bwd: gq = g z (1 - q^2), gz = g (q - h) z (1 - z), dense [pix][hidden]; rows (may be NULL)
 *   [stx_convgru_gate_rows(P, hidden)][2][hidden] per-workgroup partial sums of gq | gz (the bias gradients).
 * stx_convgru_reset_bwd: buf [pix][buf_pitch] holds g_rh in its first `hidden` channels: gr = g_rh h r (1 - r), and these
 *   channels become g (1 - z) + g_rh r; rows (may be NULL) [stx_convgru_gate_rows][hidden] partial sums of gr.
 * stx_convgru_row_sum: out[n] = sum of rows[nrows][n] in row order.
 * stx_convgru_wgrad: dw[(1 or 2) CG][K][9] from the source list against the dense maps g0 (and g1, may be NULL) [pix][CG];
 *   partial sums in `workspace` (stx_convgru_wgrad_workspace_floats(B, H, W, K, CC = rows of dw) floats), fixed-order reduction.
 * No atomics: every result is bitwise reproducible.  Unsupported arguments return an error (the queries 0) and launch nothing. */
int stx_convgru_supported(int hidden, int nx, int cx0, int cx1, int cx2, int ksize);
long long stx_convgru_packed_floats(int K, int N);
int stx_convgru_pack_weight(const float* w0, const float* w1, float* wp, int A, int Bd, int mode, void* stream);
int stx_convgru_gemm(const float* s0, int c0, int p0, const float* s1, int c1, int p1, const float* s2, int c2, int p2,
                     const float* s3, int c3, int p3, const float* wp, int N, int epi, int split, const float* bias0,
                     const float* bias1, const float* add0, int add0_pitch, const float* add1, int add1_pitch, const float* h,
                     int h_pitch, const float* z, float* out0, float* out1, float* out2, int out_pitch, int B, int H, int W,
                     void* stream);
int stx_convgru_gate_rows(long long P, int hidden);
int stx_convgru_gate_bwd(const float* g, int g_pitch, const float* z, const float* q, const float* h, int h_pitch, float* gq,
                         float* gz, float* rows, long long P, int hidden, void* stream);
int stx_convgru_reset_bwd(float* buf, int buf_pitch, const float* g, int g_pitch, const float* z, const float* r, const float* h,
                          int h_pitch, float* gr, float* rows, long long P, int hidden, void* stream);
int stx_convgru_row_sum(const float* rows, float* out, int nrows, int n, void* stream);
long long stx_convgru_wgrad_workspace_floats(int B, int H, int W, int K, int CC);
int stx_convgru_wgrad(const float* s0, int c0, int p0, const float* s1, int c1, int p1, const float* s2, int c2, int p2,
                      const float* s3, int c3, int p3, const float* g0, const float* g1, int CG, float* dw, float* workspace,
                      int B, int H, int W, void* stream);

/* ---- Selective recurrent unit (csrc/selgru.hip) ------------------------------------------------------
 * SelectiveConvGRU of SelectiveStereo (reference SelectiveStereo/SelectiveRAFT/update.py:15-71, the same text in SelectiveIGEV):
 * h' = att h_s + (1 - att) h_l with h_s a RaftConvGRU of 1x1 kernels and h_l one of 3x3 kernels (the 3x3 cell is the stx_convgru_*
 * entry points with NULL context biases).  These entry points are the 1x1 cell, the blend and its gradient.  Layout, the SOURCE
 * lists and the limits are those of the ConvGRU block above (stx_selgru_supported(hidden, nx, cx0, cx1, cx2)); a 1x1 kernel sees
 * no neighbours, so the pixels are one flat axis of P = B H W.
 * stx_selgru_pack_weight: packs one or two (w1 may be NULL) torch weights [A][Bd][1][1], stacked along A, into
 *   stx_selgru_packed_floats(K, N) floats; mode 0: forward (K = Bd, N = A or 2 A); mode 1: data gradient (transposed channels:
 *   K = A or 2 A, N = Bd).
 * stx_selgru_gemm: acc[pix][n] = sum over the source list with packed weights of N output channels, then the epilogue `epi`:
 *   0 raw: out0[pix][out_pitch] = (acc + add0[pix][add0_pitch]) + add1[pix][add1_pitch] (each may be NULL; out0 may be either);
 *   1 zr:  N = 2 split (split = hidden): out0 = z = sigmoid(acc + bias0), out1 = r h with r = sigmoid(acc + bias1), out2 = r
 *          (may be NULL);
 *   2 q:   N = split: q = tanh(acc + bias0), mine = (1 - z) h + z q, out1 = q (may be NULL), and with `blend`
 *          0: out0 = mine;  1: out0 = att mine + (1 - att) other;  2: out0 = att other + (1 - att) mine
 *          (att [pix], other [pix][hidden] = the other cell's state; out0 may be `other`: the blend is formed in place).
 *   Pre-activations, gates, the convex update and the blend are formed in double and rounded once.  Outputs never alias h.
 * stx_selgru_blend_bwd: gs = att g, gl = (1 - att) g dense [pix][hidden]; gatt (may be NULL) [pix] = sum_c g (h_s - h_l) with
 *   h_s, h_l re-formed from zs, qs, zl, ql and h, summed in double in channel order.
 * stx_selgru_wgrad: dw[(1 or 2) CG][K] from the source list against the dense maps g0 (and g1, may be NULL) [pix][CG]; partial
 *   sums in `workspace` (stx_selgru_wgrad_workspace_floats(P, K, CC = rows of dw) floats), fixed-order reduction.
 * stx_selgru_col_sum: out[k][n] = column sums of up to three dense maps [pix][n] (trailing ones may be NULL), in double, rounded
 *   once: the bias gradients from gq, gz, gr; `workspace` of stx_selgru_col_sum_workspace_floats(P, n) floats, 8-byte aligned.
 * The gate / reset backward of a 1x1 cell are stx_convgru_gate_bwd / _reset_bwd (their partial rows may be NULL).
 * No atomics: every result is bitwise reproducible.  Unsupported arguments return an error (the queries 0) and launch nothing. */
int stx_selgru_supported(int hidden, int nx, int cx0, int cx1, int cx2);
long long stx_selgru_packed_floats(int K, int N);
int stx_selgru_pack_weight(const float* w0, const float* w1, float* wp, int A, int Bd, int mode, void* stream);
int stx_selgru_gemm(const float* s0, int c0, int p0, const float* s1, int c1, int p1, const float* s2, int c2, int p2,
                    const float* s3, int c3, int p3, const float* wp, int N, int epi, int split, const float* bias0,
                    const float* bias1, const float* add0, int add0_pitch, const float* add1, int add1_pitch, const float* h,
                    int h_pitch, const float* z, const float* att, const float* other, int blend, float* out0, float* out1,
                    float* out2, int out_pitch, long long P, void* stream);
int stx_selgru_blend_bwd(const float* g, int g_pitch, const float* att, const float* zs, const float* qs, const float* zl,
                         const float* ql, const float* h, int h_pitch, float* gs, float* gl, float* gatt, long long P, int hidden,
                         void* stream);
long long stx_selgru_col_sum_workspace_floats(long long P, int n);
int stx_selgru_col_sum(const float* m0, const float* m1, const float* m2, float* out, double* workspace, long long P, int n,
                       void* stream);
long long stx_selgru_wgrad_workspace_floats(long long P, int K, int CC);
int stx_selgru_wgrad(const float* s0, int c0, int p0, const float* s1, int c1, int p1, const float* s2, int c2, int p2,
                     const float* s3, int c3, int p3, const float* g0, const float* g1, int CG, float* dw, float* workspace,
                     long long P, void* stream);

/* ---- Contextual spatial attention (csrc/csa.hip) -----------------------------------------------------
 * ChannelAttentionEnhancement and SpatialAttentionExtractor of SelectiveStereo (reference SelectiveStereo/SelectiveRAFT/update.py:
 * 106-135), used as `x' = cam(x) x; att = sam(x')`: gate = sigmoid(W2 relu(W1 avg) + W2 relu(W1 max)) over the global average /
 * max pools of x, W1 [C/16][C], W2 [C][C/16]; att = sigmoid(conv_kxk([mean_c x' | max_c x'])) with w [2][k][k], zero padding k / 2.
 * x is channels-last fp32 [B][HW][pitch >= C]; served (stx_csa_supported(C, k)): C a multiple of 16 up to 256, k odd up to 7.
 * All sums and products are formed in double and rounded once.  Ties of a max go to the lowest pixel (global pool) / the lowest
 * channel (per pixel).  No atomics: partials per workgroup, combined in a fixed order.
 * stx_csa_pool:  partials psum (double) / pmax / pidx [B][nblk][C], nblk = stx_csa_blocks(HW, C).
 * stx_csa_gate:  the gate [B][C] from the partials by one workgroup per batch item, with pooled [B][2][C] (double, avg | max) and
 *   argp [B][C] (arg max pixel) for the backward pass.
 * stx_csa_apply: xp = x' = gate x dense [B][HW][C], map [B][HW][2] = channel mean | max of x', argc [B][HW] the arg max channel
 *   (may be NULL); every workgroup recomputes the gate from the partials; gate / pooled / argp (all or none) as stx_csa_gate
 *   leaves them.  With w1 NULL there is no gate: map / argc are those of x itself.
 * stx_csa_sam:   att [B][H][W] from map and w.
 * stx_csa_sam_bwd: from g = dL/d att: gpre (scratch [B][H][W]), gmap [B][H][W][2] and dw [2][k][k] (may be NULL; else `workspace`
 *   of stx_csa_sam_bwd_workspace_floats floats, 8-byte aligned).
 * stx_csa_apply_bwd: g_x' = gxp (may be NULL) + the map's gradient gmap through mean and arg max (may be NULL, else with argc);
 *   gx = gate g_x' dense [B][HW][C] (gate NULL: g_x'), pgate (may be NULL) [B][nblk][C] doubles = partial sums of g_x' x.
 * stx_csa_gate_bwd: one workgroup: from the gate's gradient -- the partials pgate, or gg [B][C] floats -- and pooled: dw1, dw2 (may
 *   be NULL), gavg [B][C] (per pixel, 1 / HW folded in) and gmx [B][C] (to the arg max pixel).
 * stx_csa_pool_bwd: gx[b][pix][c] (+)= gavg + (pix == argp) gmx. */
int stx_csa_supported(int C, int ksize);
int stx_csa_blocks(long long HW, int C);
int stx_csa_pool(const float* x, int pitch, double* psum, float* pmax, int* pidx, int B, long long HW, int C, void* stream);
int stx_csa_gate(const double* psum, const float* pmax, const int* pidx, int nblk, const float* w1, const float* w2, float* gate,
                 double* pooled, int* argp, int B, long long HW, int C, void* stream);
int stx_csa_apply(const float* x, int pitch, const double* psum, const float* pmax, const int* pidx, int nblk, const float* w1,
                  const float* w2, float* xp, float* map, int* argc, float* gate, double* pooled, int* argp, int B, long long HW,
                  int C, void* stream);
int stx_csa_sam(const float* map, const float* w, float* att, int B, int H, int W, int ksize, void* stream);
long long stx_csa_sam_bwd_workspace_floats(int B, int H, int W, int ksize);
int stx_csa_sam_bwd(const float* g, const float* att, const float* map, const float* w, float* gpre, float* gmap, float* dw,
                    double* workspace, int B, int H, int W, int ksize, void* stream);
int stx_csa_apply_bwd(const float* x, int pitch, const float* gate, const float* gxp, int gxp_pitch, const float* gmap,
                      const int* argc, float* gx, double* pgate, int B, long long HW, int C, void* stream);
int stx_csa_gate_bwd(const double* pgate, int nblk, const float* gg, const double* pooled, const float* w1, const float* w2,
                     float* dw1, float* dw2, float* gavg, float* gmx, int B, long long HW, int C, void* stream);
int stx_csa_pool_bwd(float* gx, const float* gavg, const float* gmx, const int* argp, int accumulate, int B, long long HW, int C,
                     void* stream);

/* 3x3 stride-1 Conv2d (padding 1, no bias), channels-last, of the 2-D feature CNN's BasicBlocks with 32 / 64 channels: forward
 * and data gradient (reference models/GwcNet/gwcnet.py:12-42 `convbn(in, out, 3, 1, pad, 1)` -> nn.Conv2d at 1/2 and 1/4
 * resolution; PSMNet/submodule.py:57-97; ACVNet/acv.py:15-40).  x [B][H][W][Cin], out [B][H][W][Cout], fp32.
 * w = the layer's parameter [Co_w][Ci_w][3][3] in channels_last storage = dense [Co_w][3][3][Ci_w], read by the kernel as it is
 * (no packing step).  dgrad = 0: out = conv(x, w), Cin = Ci_w, Cout = Co_w.  dgrad = 1: the input gradient of that layer,
 * x = the output gradient, Cin = Co_w, Cout = Ci_w (flipped taps, transposed channels).
 * stats (may be NULL): [stx_conv2d_stat_rows(groups)][2][Cout] per-workgroup sum / sum of squares of the raw output, the batch
 *   split into `groups` equal parts (views) with their own rows: rows [g * rows / groups, (g + 1) * rows / groups) belong to part g
 *   -> stx_bn_finalize_groups.  Shapes: stx_conv2d_supported (Cin 32 or 64, Cout % 16 == 0). */
int stx_conv2d_supported(int Cin, int Cout);
long long stx_conv2d_stat_rows(int groups);
int stx_conv2d_fwd(const float* x, const float* w, float* out, float* stats, int B, int H, int W, int Cin, int Cout, int dgrad,
                   int groups, void* stream);

/* Classifier tail Conv3d(Cin, 1, k=3, p=1, bias=False) (GwcNet/gwcnet.py:139-153, PSMNet/stackhourglass.py:74-84):
 * N = 1 is not GEMM-shaped, so it gets VALU kernels. w: torch layout [1][Cin][27]; out/residual/gy: [B][D][H][W].
 * Cin % 16 == 0 (wgrad: Cin <= 64). dgrad: gx [B][D][H][W][Cin] = autograd input gradient of the same layer
 * (Cin % 4 == 0, Cin <= 64); a streaming kernel: reads the 1-channel gy, writes Cin channels. */
int stx_conv3d_c1_fwd(const float* x, const float* w, const float* residual, float* out, int B, int D, int H, int W,
                      int Cin, void* stream);
long long stx_conv3d_c1_wgrad_workspace_floats(int Cin);
int stx_conv3d_c1_wgrad(const float* x, const float* gy, float* dw, float* workspace, int B, int D, int H, int W,
                        int Cin, void* stream);
int stx_conv3d_c1_dgrad(const float* gy, const float* w, float* gx, int B, int D, int H, int W, int Cin, void* stream);

/* Mish activation y = x * tanh(softplus(x)) (models/PCWNet/submodule.py:11-18,178-190): n floats, n % 4 == 0, in place allowed;
 * backward gx = gy * mish'(x) with x the activation input. */
int stx_mish_fwd(const float* x, float* y, long long n, void* stream);
int stx_mish_bwd(const float* gy, const float* x, float* gx, long long n, void* stream);
/* IGEV-family cost aggregation (models/IGEVStereo/igev_stereo.py:23-100).
 * stx_depth_to_space: the interleave of ConvTranspose3d(k=4, s=2, p=1)'s eight output-parity classes (igev_stereo.py:44-51):
 * the transposed convolution runs as ONE 3x3x3 stride-1 convolution with 8*C class-major output channels on stx_conv3d_fwd
 * (each class: its 8 taps in a zero-filled 27-tap set); y [B][D][H][W][8C] -> out [B][2D][2H][2W][C],
 * out[2d+pd][2h+ph][2w+pw][c] = y[d][h][w][(4pd+2ph+pw)C + c]; inverse != 0 maps the other way (its backward).  C % 4 == 0. */
int stx_depth_to_space(const float* y, float* out, int B, int D, int H, int W, int C, int inverse, void* stream);
/* FeatureAtt (models/IGEVStereo/submodule.py:228-241): out = cv * sigmoid(att), the gate att [B][HW][C] broadcast over the
 * disparity axis of cv / out [B][D][HW][C]; backward: gcv = g * sigmoid(att), gatt = sum_d g * cv * s (1 - s) (either may be
 * NULL).  C % 4 == 0. */
int stx_gate_fwd(const float* cv, const float* att, float* out, int B, int D, long long HW, int C, void* stream);
int stx_gate_bwd(const float* g, const float* cv, const float* att, float* gcv, float* gatt, int B, int D, long long HW,
                 int C, void* stream);

/* ---- channel concatenation of channels-last activations --------------------------------------------------
 * Replaces `torch.cat((l2, l3, l4), dim=1)` of the feature extractors (reference models/GwcNet/gwcnet.py:59,
 * models/ACVNet/acv.py:48) for dense [nvox][C_k] (NHWC / NDHWC) tensors: out[v] = in0[v] | in1[v] | in2[v] | in3[v]; unused
 * parts: NULL with C = 0; every C_k a multiple of 4.  stx_split_channels is the inverse (the concatenation's backward); a
 * part with C_k > 0 must have a destination. */
int stx_concat_channels(const float* in0, const float* in1, const float* in2, const float* in3, int C0, int C1, int C2, int C3,
                        float* out, long long nvox, void* stream);
int stx_split_channels(const float* in, float* out0, float* out1, float* out2, float* out3, int C0, int C1, int C2, int C3,
                       long long nvox, void* stream);
/* Batched 2-D transpose out[n][c][r] = in[n][r][c]: the channels-last <-> channel-major re-layout of the feature maps in front
 * of the cost-volume builders (their kernels take NCHW rows, the 2-D CNN produces NHWC; `Tensor.contiguous()` in the reference's
 * terms).  rows and cols multiples of 4. */
int stx_transpose(const float* in, float* out, int N, int rows, int cols, void* stream);

/* ---- ACVNet extras (models/ACVNet/acv.py) --------------------------------------------------------------
 * Depth-wise nn.Conv3d(C, C, (1,3,3), groups=C, dilation=d, padding=(0,d,d)) (acv.py:109-112,183-187) on a channels-last
 * volume; `dil` = int[C/4] dilation per channel quad (device pointer); w = [C][9]; flip=1 mirrors the taps (input gradient). */
int stx_dwconv_hw_fwd(const float* x, const float* w, const int* dil, float* out, int B, int D, int H, int W, int C,
                      int flip, void* stream);
long long stx_dwconv_hw_wgrad_workspace_floats(int C);
int stx_dwconv_hw_wgrad(const float* x, const float* gy, const int* dil, float* dw, float* workspace, int B, int D,
                        int H, int W, int C, void* stream);
/* gradient of `softmax(att, dim=2) * concat_volume` (acv.py:196) w.r.t. the probabilities:
 * gscale[b][d][h][w] = sum_c gvol[b][d][h][w][c] * concat[b][d][h][w][c]; gvol has 2*Cc channels */
int stx_cost_volume_scale_bwd(const float* gvol, const float* Lc, const float* Rc, float* gscale, int B, int Cc, int H,
                              int W, int D, int mask_left, void* stream);
/* out[v][c] = x[v][c] * s[v] over [nvox][C] */
int stx_scale_channels(const float* x, const float* s, float* out, long long nvox, int C, void* stream);
/* Backward of the attention concat volume vol = prob * concat(L, R shifted) (models/ACVNet/acv.py:196 with
 * ACVNet/submodule.py:180-191) in one pass over gvol [B][D][H][W][2 Cc]: gL, gR [B][Cc][H][W], gprob [B][D][H][W].
 * D * W * 4 bytes must fit in 150 KiB of LDS (else: bad-argument error; use stx_cost_volume_scale_bwd +
 * stx_scale_channels + stx_cost_volume_bwd). */
int stx_ac_volume_bwd(const float* gvol, const float* Lc, const float* Rc, const float* prob, float* gL, float* gR,
                      float* gprob, int B, int Cc, int H, int W, int D, int mask_left, void* stream);

/* ---- train-mode BatchNorm3d (+ReLU / residual) around the convolutions ---------------------------------
 * nn.BatchNorm3d of convbn_3d (models/GwcNet/submodule.py:17-20) in train() mode and the adds/ReLUs that follow it
 * (GwcNet/gwcnet.py:96-103,185; PSMNet/stackhourglass.py:31-48). */
int stx_bn_reduce_blocks(void);
/* Batch statistics of a channels-last activation z [nvox][C] whose producer has no fused epilogue -- the nn.BatchNorm2d
 * layers behind the MIOpen convolutions of the 2-D feature CNN (models/GwcNet/gwcnet.py:12-65 `convbn`, BasicBlock):
 * partials [stx_bn_stats_rows(nvox, C)][2][C] = per-workgroup (sum z, sum z^2), the row format stx_bn_finalize takes.
 * C: multiple of 4 with C/4 dividing 256.
 * GROUPS (here and in stx_bn_apply / stx_bn_bwd_reduce2 / stx_bn_bwd_apply2): the tensors are `groups` consecutive slabs of
 * `nvox` voxels, each with its OWN statistics -- the per-group vectors (partials, scale, shift, mean, invstd, sums) are
 * [groups][...], gamma is shared.  The 2-D CNN sends the left and the right view through its convolutions as one batch
 * while every BatchNorm keeps the per-view statistics of the reference's two extractor calls (gwcnet.py:172-173). */
int stx_bn_stats_rows(long long nvox, int C);
int stx_bn_stats(const float* z, float* partials, long long nvox, int C, int groups, void* stream);
/* partials [nrows][2][C] (from the conv epilogue) -> scale = gamma*invstd, shift = beta - mean*scale, mean, invstd;
 * running_mean/var (may be NULL) updated with `momentum` and the unbiased variance, like torch. */
int stx_bn_finalize(const float* partials, int nrows, int C, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                    float* mean, float* invstd, void* stream);
/* The same for `groups` slabs of a batch with their own statistics in ONE launch: partials [groups][nrows][2][C],
 * count = voxels per slab, out [4][groups][C] = scale, shift, mean, invstd.  The running statistics are updated slab
 * after slab, in order -- bit-identical to `groups` calls of stx_bn_finalize (the two views of the 2-D feature CNN:
 * reference models/GwcNet/gwcnet.py:172-173 runs the extractor once per view). */
int stx_bn_finalize_groups(const float* partials, int nrows, int C, double count, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, float* out, int groups,
                           void* stream);
/* out = act(z1*scale1+shift1 [+ z2*scale2+shift2 | + z2 when scale2 == NULL]) over [nvox][C]; `relu` = activation code
 * (0 none, 1 ReLU, 2 Mish, 3 LeakyReLU(0.01)) here and in the backward passes below; Mish is differentiated at the pre-activation value,
 * which stx_bn_bwd_reduce2 / _apply2 recompute from z and the scale / shift vectors (y = NULL) */
int stx_bn_apply(const float* z1, const float* scale1, const float* shift1, const float* z2, const float* scale2,
                 const float* shift2, float* out, long long nvox, int C, int relu, int groups, void* stream);
/* sums[3][C] = sum g, sum g*xhat1, sum g*xhat2 with g = gy*[y>0]; partials: scratch of stx_bn_reduce_blocks()*3*C floats */
int stx_bn_bwd_reduce(const float* gy, const float* y, const float* z1, const float* mean1, const float* invstd1,
                      const float* z2, const float* mean2, const float* invstd2, float* partials, float* sums,
                      long long nvox, int C, int relu, void* stream);
/* dz_k = gamma_k*invstd_k*(g - sums[0]/N - xhat_k*sums[k]/N); gout (may be NULL) receives g for a plain residual branch */
int stx_bn_bwd_apply(const float* gy, const float* y, const float* z1, const float* mean1, const float* invstd1,
                     const float* gamma1, const float* z2, const float* mean2, const float* invstd2,
                     const float* gamma2, const float* sums, float* dz1, float* dz2, float* gout, long long nvox, int C,
                     int relu, void* stream);
/* The same two passes taking the ReLU mask from the forward pass's per-channel scale / shift instead of the activated
 * output (y may be NULL): sign(y) = sign(fmaf(z1, scale1, shift1) [+ fmaf(z2, scale2, shift2)]) is recomputed from
 * operands these passes read anyway -- one volume-sized read less per pass.  (A block with a plain residual still passes y.)
 * With groups > 1 `sums` holds groups + 1 slabs of [3][C]: the per-group sums, then their total over the groups (the gradients
 * of the gamma / beta the groups share); stx_bn_bwd_apply2 reads the first `groups` slabs. */
int stx_bn_bwd_reduce2(const float* gy, const float* y, const float* z1, const float* mean1, const float* invstd1,
                       const float* z2, const float* mean2, const float* invstd2, const float* scale1,
                       const float* shift1, const float* scale2, const float* shift2, float* partials, float* sums,
                       long long nvox, int C, int relu, int groups, void* stream);
int stx_bn_bwd_apply2(const float* gy, const float* y, const float* z1, const float* mean1, const float* invstd1,
                      const float* gamma1, const float* z2, const float* mean2, const float* invstd2,
                      const float* gamma2, const float* scale1, const float* shift1, const float* scale2,
                      const float* shift2, const float* sums, float* dz1, float* dz2, float* gout, long long nvox,
                      int C, int relu, int groups, void* stream);

/* ---- Evaluation-path input step on the device --------------------------------------------------------
 * pad_to_2x (datasets/data_augmentation/__init__.py:57-80: zero padding on top and to the right, to multiples of 96)
 * + get_transform (datasets/utils.py:62-69: torchvision ToTensor and Normalize) of one view, fused:
 *   img uint8 [B][H][W][3] -> out fp32 [B][3][Hp][Wp],  out = ((inside ? img : 0) / 255 - mean[c]) / std[c],
 * top = Hp - H rows of padding above the image, Wp - W columns to its right; mean3 / std3 are HOST arrays of 3 floats.
 * Bit-identical to the reference arithmetic (IEEE fp32 division by 255, subtraction, division by std). */
int stx_pad_normalize_u8(const unsigned char* img, float* out, int B, int H, int W, int Hp, int Wp, int top,
                         const float* mean3, const float* std3, void* stream);

/* ---- Sampled (cascade) cost volume of the CFNet family ---------------------------------------------------
 * One call replaces, per cascade stage (models/CFNet/cfnet.py:553-566 / 584-597),
 *   SpatialTransformer (models/CFNet/submodule.py:306-350) x 2, groupwise_correlation_4D (submodule.py:163-169),
 *   cost_volume_generator (cfnet.py:470-497) x 2 and torch.cat((gwc_volume, concat_volume, disparity_samples), dim=1):
 *   vol[b][s][h][w][:] = ( mean_c Lg[g*cpg+c][h][w] * Rg[g*cpg+c][h][x]   g < G
 *                        | Lc[c][h][w] | Rc[c][h][x]                        c < Cc
 *                        | samples[b][s][h][w] | zero pad up to CTp ),     x = w - samples[b][s][h][w]
 * with the reference's boundary rule: the gather index is clamped into the row and every right-feature term is
 * zeroed where the un-clamped x leaves [0, W-1].  Features NCHW fp32, samples [B][S][H][W] (integer-valued floats),
 * vol NDHWC [B][S][H][W][CTp], CTp >= G + 2*Cc + 1 and a multiple of 4 (the consuming convolution wants 8).
 * _bwd: gradients w.r.t. the four feature maps (the hypotheses carry none); gRg / gRc are zeroed and then accumulated
 * with float atomics, like the reference's gather backward. */
int stx_sampled_volume_fwd(const float* Lg, const float* Rg, int Cg, int G, const float* Lc, const float* Rc, int Cc,
                           const float* samples, float* vol, int B, int H, int W, int S, int CTp, void* stream);
int stx_sampled_volume_bwd(const float* gvol, const float* Lg, const float* Rg, int Cg, int G, int Cc,
                           const float* samples, float* gLg, float* gRg, float* gLc, float* gRc, int B, int H, int W,
                           int S, int CTp, void* stream);

/* ---- refine2d.hip: 2-D helpers of the PCWNet / CFNet family -------------------------------------
 * warp(x, disp) (models/PCWNet/submodule.py:137-176): x [B][C][H][W] (right-view features), disp [B][1][H][W] ->
 * out [B][C][H][W] = grid_sample(x, grid(w - disp, h)) (bilinear, zeros outside, the reference's (W-1)/(H-1) grid under
 * align_corners=False) * (in-image weight sum >= 0.999).  Backward: gx (cleared inside, float atomics like torch's own
 * grid-sampler backward; may be NULL) and gdisp [B][1][H][W] (may be NULL); the validity mask is a constant. */
int stx_warp_fwd(const float* x, const float* disp, float* out, int B, int C, int H, int W, void* stream);
int stx_warp_bwd(const float* gout, const float* x, const float* disp, float* gx, float* gdisp, int B, int C, int H, int W,
                 void* stream);
/* build_corrleation_volume(ref, tgt, maxdisp, groups) (models/PCWNet/submodule.py:121-135, dup CFNet/submodule.py:181-195):
 * ref, tgt [B][C][H][W] -> vol [B][groups][2*maxdisp+1][H][W]; slice maxdisp+i, i >= 0: mean over the group's channels of
 * ref[w] * tgt[w-i] at w >= i, 0 elsewhere; slice maxdisp-n, n >= 1 (literal semantics of the reference's `[..., :-i]` with
 * negative i): the FIRST n columns of ref against the LAST n columns of tgt, 0 elsewhere.  Every element of vol is written.
 * maxdisp <= min(48, W).  Backward: gref / gtgt [B][C][H][W] fully written (either may be NULL), deterministic. */
int stx_corr_volume_fwd(const float* ref, const float* tgt, float* vol, int B, int C, int H, int W, int maxdisp, int groups,
                        void* stream);
int stx_corr_volume_bwd(const float* gvol, const float* ref, const float* tgt, float* gref, float* gtgt, int B, int C, int H,
                        int W, int maxdisp, int groups, void* stream);
/* disparity_variance(x, maxdisp, disparity) (models/CFNet/submodule.py:128-134; samples == NULL): out[b][i] =
 * sum_d x[b][d][i] * (d - disp[b][i])^2, and disparity_variance_confidence(x, samples, disparity) (:136-140; samples
 * [B][D][HW]): sum_d x * (disp - samples)^2.  x [B][D][HW], disp / out [B][HW].  Backward: gx, gdisp, gsamples (each may
 * be NULL). */
int stx_disparity_variance_fwd(const float* x, const float* disp, const float* samples, float* out, int B, int D, int HW,
                               void* stream);
int stx_disparity_variance_bwd(const float* g, const float* x, const float* disp, const float* samples, float* gx, float* gdisp,
                               float* gsamples, int B, int D, int HW, void* stream);

/* ---- geo_lookup.hip: geometry-encoding lookup and convex upsampling of the IGEV family ---------------------------------
 * Combined_Geo_Encoding_Volume (models/IGEVStereo/geometry.py:7-70; called once per GRU iteration, igev_stereo.py:229-239) and
 * context_upsample (models/IGEVStereo/submodule.py:243-255; igev_stereo.py:164,254).
 * PYRAMIDS are pixel-major, the levels one behind the other in one buffer: level i of a pyramid over `rows` rows of `len`
 * positions with C channels is [rows][len >> i][C] (avg_pool2d([1,2]) of level i-1 along `len`, an odd tail dropped) and the
 * whole pyramid has stx_geo_pyramid_floats(rows, len, C, levels) floats.  Geometry pyramid: rows = B*H*W pixels, len = D;
 * correlation pyramid: rows = B*H*W1, len = W2, C = 1.  levels 1..3.
 * stx_geo_corr_fwd: all-pairs row correlation corr[b][h][w1][w2] = sum_c fmap1[b][c][h][w1] * fmap2[b][c][h][w2]
 *   (geometry.py:62-70) on the matrix cores AND its pooled levels, into cpyr; fmap1 [B][C][H][W1], fmap2 [B][C][H][W2], any C.
 * stx_geo_corr_bwd: gcpyr (gradient of every level) -> gfmap1, gfmap2 (either may be NULL); every element written.
 * stx_geo_pyramid_fwd: vol dense [B][D][H][W][C] (C % 4 == 0) -> gpyr, all levels in one launch; _bwd: the inverse, gvol
 *   fully written.  D * 17 * C floats must fit 64 KiB of LDS at a tile of 16 pixels (narrower tiles are used beyond that). */
long long stx_geo_pyramid_floats(long long rows, int len, int C, int levels);
int stx_geo_corr_fwd(const float* fmap1, const float* fmap2, float* cpyr, int B, int C, int H, int W1, int W2, int levels,
                     void* stream);
int stx_geo_corr_bwd(const float* gcpyr, const float* fmap1, const float* fmap2, float* gfmap1, float* gfmap2, int B, int C, int H,
                     int W1, int W2, int levels, void* stream);
int stx_geo_pyramid_fwd(const float* vol, float* gpyr, int B, int D, int H, int W, int C, int levels, void* stream);
int stx_geo_pyramid_bwd(const float* ggpyr, float* gvol, int B, int D, int H, int W, int C, int levels, void* stream);
/* The lookup (geometry.py:35-59): disp, coords [B*H*W] (coords = the pixel's own column in the reference);
 * out [B][levels * (C + 1) * (2 radius + 1)][H][W], per level first channel c * (2 radius + 1) + k for the C geometry channels
 * sampled at disp / 2^i + k - radius, then the 2 radius + 1 samples of the pixel's correlation row at
 * (coords - disp) / 2^i + k - radius; linear interpolation, taps outside the level read as zero.  radius 1..8; the
 * correlation rows have W1 = W.
 * _bwd: gout -> ADDED (+=) to ggpyr / gcpyr (either may be NULL), which the caller clears before the first of the lookups
 * whose gradients it wants summed; a pixel touches only its own rows: no atomics, bitwise reproducible.  disp and coords
 * carry no gradient (the reference detaches disp, igev_stereo.py:238). */
int stx_geo_lookup_fwd(const float* gpyr, const float* cpyr, const float* disp, const float* coords, float* out, int B, int H,
                       int W, int D, int C, int W2, int levels, int radius, void* stream);
int stx_geo_lookup_bwd(const float* gout, const float* disp, const float* coords, float* ggpyr, float* gcpyr, int B, int H, int W,
                       int D, int C, int W2, int levels, int radius, void* stream);
/* context_upsample: disp_low [B][1][h][w], up_weights [B][9][4h][4w] -> out [B][4h][4w],
 * out[4y+j][4x+i] = sum_t up_weights[t][4y+j][4x+i] * disp_low[y + t/3 - 1][x + t%3 - 1] (zero padding), no unfolded or
 * up-sampled temporary.  _bwd: g [B][4h][4w] -> gdisp [B][1][h][w] (needs up_weights) and gweights [B][9][4h][4w] (needs
 * disp_low); either may be NULL; deterministic. */
int stx_context_upsample_fwd(const float* disp_low, const float* up_weights, float* out, int B, int h, int w, void* stream);
int stx_context_upsample_bwd(const float* g, const float* disp_low, const float* up_weights, float* gdisp, float* gweights, int B,
                             int h, int w, void* stream);

/* ---- corr1d.hip: all-pairs 1-D correlation pyramid and lookup of the RAFT family -----------------------------------------
 * CorrBlock1D / CorrBlockFast1D / PytorchAlternateCorrBlock1D (models/RAFTStereo/corr.py:31-156, utils/utils.py:59-74; used
 * unchanged by Selective-RAFT) and the disparity-indexed CorrBlock1D of DEFOM-Stereo (models/DEFOMStereo/corr.py:113-181).
 * The PYRAMID is pixel-major like the correlation pyramid above: level i is [B*H*W1][W2 >> i], the levels one behind the other,
 * stx_corr1d_pyramid_floats(B*H*W1, W2, levels) floats in all; levels 1..4, and the last level must keep at least 2 positions
 * (the reference normalises by length - 1).
 * stx_corr1d_pyramid_fwd: level 0 = scale * sum_c fmap1[b][c][h][w1] * fmap2[b][c][h][w2] on the matrix cores (the reference's
 *   scale is 1 / sqrt(C)) AND the pooled levels, one launch; fmap1 [B][C][H][W1], fmap2 [B][C][H][W2], any C.
 * stx_corr1d_pyramid_bwd: gcpyr (gradient of every level) -> gfmap1, gfmap2 (either may be NULL); every element written.
 * The lookup: `jobs` is a HOST array of njobs x 4 floats (level, radius, alpha, mult), njobs 1..8, radius 1..8.  Per pixel p,
 *   job j writes the 2 radius + 1 samples of p's row of its level at x = (base[p] - alpha * disp[p]) * mult + k, k = -radius ..
 *   radius (linear interpolation, zero outside the row), to the channels after those of the jobs before it:
 *   out [B][sum_j (2 radius_j + 1)][H][W1].  base, disp: [B*H*W1]; disp may be NULL (then alpha is not used).
 *   RAFT: (i, r, 0, 2^-i), base = coords[:, 0].  DEFOM: (i, r, 1, 2^-i); scaling: (0, r_s, s, 1) per s of scale_list.
 * _bwd: gout -> ADDED (+=) to gcpyr, which the caller clears before the first of the lookups whose gradients it wants
 *   summed; a pixel touches only its own rows: no atomics, bitwise reproducible.  base and disp carry no gradient (the
 *   reference detaches them: raft_stereo.py:154, defom_stereo.py:142). */
long long stx_corr1d_pyramid_floats(long long rows, int W2, int levels);
int stx_corr1d_pyramid_fwd(const float* fmap1, const float* fmap2, float* cpyr, int B, int C, int H, int W1, int W2, int levels,
                           float scale, void* stream);
int stx_corr1d_pyramid_bwd(const float* gcpyr, const float* fmap1, const float* fmap2, float* gfmap1, float* gfmap2, int B, int C,
                           int H, int W1, int W2, int levels, float scale, void* stream);
int stx_corr1d_lookup_fwd(const float* cpyr, const float* base, const float* disp, const float* jobs, int njobs, float* out, int B,
                          int H, int W1, int W2, int levels, void* stream);
int stx_corr1d_lookup_bwd(const float* gout, const float* base, const float* disp, const float* jobs, int njobs, float* gcpyr,
                          int B, int H, int W1, int W2, int levels, void* stream);

/* ---- allpairs.hip: StereoAnywhere's volume stage on a row-wise all-pairs volume vol [B][H][W1][W2] -------------------------
 * The four estimates regressed from the volume (models/StereoAnywhere/utils/utils.py:112-170), W1 != W2 allowed:
 *   p_l = softmax over w2:  disp_l [B][H][W1] = w1 - sum_w2 p_l w2,  conf_l = 1 + sum_w2 p_l log2(p_l + 1e-6) / log2(W2)
 *   p_r = softmax over w1:  disp_r [B][H][W2] = sum_w1 p_r w1 - w2,  conf_r = 1 + sum_w1 p_r log2(p_r + 1e-6) / log2(W1)
 * stx_allpairs_estimates_fwd: `which` is a mask of bits 1 (disp_l), 2 (conf_l), 4 (disp_r), 8 (conf_r); exactly the outputs it
 *   names are non-NULL, the others are NULL and cost nothing (a direction neither of whose outputs is asked for is not run).
 *   stats (NULL for a plain forward): 4 * (B*H*W1 + B*H*W2) floats, per row and then per column (max, sum of exp, first moment,
 *   entropy-slope moment); the part of a direction is written when that direction runs.  The volume is not transposed.
 * stx_allpairs_estimates_bwd: any of the four gradients may be NULL (not all); those given must belong to directions the
 *   forward that wrote `stats` ran.  gvol [B][H][W1][W2]: every element written once = row-direction + column-direction softmax
 *   Jacobian terms; no atomics, bitwise reproducible.
 * Limits of the estimates: 2 <= W1 <= 512 and 2 <= W2 <= 512 (a volume row is held in registers), B*H*W1*W2 < 2^40.
 * The volume-in correlation block (corr.py:75-132) and the truncation mask (truncate_corr_volume_v2, utils/utils.py:216-238):
 * stx_corr1d_volume_pyramid_fwd: the pyramid of corr1d.hip above (same layout, stx_corr1d_pyramid_floats(B*H*W1, W2, levels)
 *   floats, levels 1..4, last level >= 2 positions, any W1 / W2) with level 0 = vol, times
 *   (1 - c) + c * (sigmoid((w1 - tdisp) - w2) * (1 - atten) + atten), c = tconf, when tdisp / tconf [B*H*W1] are given (both or
 *   neither); the pooled levels are pairwise means of the level before; everything in one launch.
 * stx_corr1d_volume_pyramid_bwd: gcpyr (gradient of every level) -> gvol, every element written, the factor applied; tdisp and
 *   tconf carry no gradient (the reference detaches the mask, stereoanywhere.py:235).
 * stx_truncate_mask_fwd: the mask volume [B][1][H][W][W] itself, same expression; has_th != 0: c = (conf > conf_th). */
int stx_allpairs_estimates_fwd(const float* vol, int which, float* disp_l, float* conf_l, float* disp_r, float* conf_r, float* stats,
                               int B, int H, int W1, int W2, void* stream);
int stx_allpairs_estimates_bwd(const float* g_disp_l, const float* g_conf_l, const float* g_disp_r, const float* g_conf_r,
                               const float* vol, const float* stats, float* gvol, int B, int H, int W1, int W2, void* stream);
int stx_corr1d_volume_pyramid_fwd(const float* vol, const float* tdisp, const float* tconf, float atten, float* cpyr, int B, int H,
                                  int W1, int W2, int levels, void* stream);
int stx_corr1d_volume_pyramid_bwd(const float* gcpyr, const float* tdisp, const float* tconf, float atten, float* gvol, int B, int H,
                                  int W1, int W2, int levels, void* stream);
int stx_truncate_mask_fwd(const float* disp, const float* conf, int has_th, float conf_th, float atten, float* mask, int B, int H,
                          int W, void* stream);

/* ---- mono_align.hip: StereoAnywhere's mono-stereo alignment stage (stereoanywhere.py:167-235) ------------------------------
 * The bin rule of generate_masks (utils/utils.py:48-54): channel i where f32(i / N) <= mde < f32((i + 1) / N), compared in fp32;
 *   values >= 1, negative values and NaN fall in no bin.  1 <= N <= 64.
 * stx_generate_masks_fwd: mde [B][1][H][W] -> masks [B][N][H][W] as fp16 (2-byte elements, 1.0 or 0.0), every element written.
 * stx_masked_volume_fwd: vol [B][1][H][W2][W3], mde_l [B][1][H][W2], mde_r [B][1][H][W3] -> out [B][N][H][W2][W3] =
 *   volume * left_masks.unsqueeze(4) * right_masks.unsqueeze(3): out[n] = vol where both bins are n, exact zero elsewhere (also
 *   where vol is not finite).  Every element written once.  W3 <= 2048, B*N*H*W2*W3 < 2^40.
 * stx_masked_volume_bwd: g [B][N][H][W2][W3] -> gvol [B][1][H][W2][W3] = g[bin_left] where the two bins agree, else 0; one
 *   gather, no atomics.  The maps carry no gradient.
 * stx_softlrc_fwd (utils/utils.py:172-198): disp2, disp3 [B][1][H][W] -> out2 = softplus(lrc_th - |disp2 - warp(disp3)|) /
 *   log(1 + e^lrc_th) and out3 likewise, the warp bilinear in both directions with zeros outside at column
 *   (x -+ relu(d)) (W - 1) / W and row y (H - 1) / H; one launch.  lrc_th <= 20, B*H*W < 2^31.
 * stx_softlrc_bwd: g2 / g3 (either may be NULL) -> gdisp2, gdisp3 through the direct term, the sampled value and the sample
 *   coordinate (with the gate of relu); two launches, no atomics, bitwise reproducible.  workspace =
 *   stx_softlrc_bwd_workspace_floats floats, 8-byte aligned.  W <= 1024.
 * stx_weighted_lsq_fwd (utils/utils.py:345-384): per image b over its n elements, s = relu(disp): the two thresholds are
 *   torch.quantile's fp32 results (order statistics by radix select, its `lerp`), the mask t_min <= s <= t_max, weights
 *   0.9 |conf| + 0.1, m = |mde|; the five sums S_wmm, S_wm, S_w, S_wms, S_ws in double in a fixed order; scale [B], shift [B]
 *   from the 2 x 2 normal equations (determinant 0: scale 0, shift S_ws / S_w).  stats: 8 doubles per image (the five sums, the
 *   two thresholds, 0), 8-byte aligned.  One launch, one workgroup per image; n < 2^24, B <= 65535, 0 <= quantiles <= 1.
 * stx_weighted_lsq_bwd: g_scale / g_shift [B] (either may be NULL) and the forward's stats -> g_mde, g_disp, g_conf [B][n],
 *   every element written; the thresholds carry no gradient.
 * stx_mirror_detector_fwd / _bwd (utils/utils.py:255-269): elementwise over n pixels; the backward writes all four gradients. */
int stx_generate_masks_fwd(const float* mde, void* masks, int B, int N, int H, int W, void* stream);
int stx_masked_volume_fwd(const float* vol, const float* mde_l, const float* mde_r, float* out, int B, int N, int H, int W2, int W3,
                          void* stream);
int stx_masked_volume_bwd(const float* g, const float* mde_l, const float* mde_r, float* gvol, int B, int N, int H, int W2, int W3,
                          void* stream);
int stx_softlrc_fwd(const float* disp2, const float* disp3, float lrc_th, float* out2, float* out3, int B, int H, int W,
                    void* stream);
long long stx_softlrc_bwd_workspace_floats(int B, int H, int W);
int stx_softlrc_bwd(const float* g2, const float* g3, const float* disp2, const float* disp3, float lrc_th, void* workspace,
                    float* gdisp2, float* gdisp3, int B, int H, int W, void* stream);
int stx_weighted_lsq_fwd(const float* mde, const float* disp, const float* conf, float min_quantile, float max_quantile, float* scale,
                         float* shift, void* stats, int B, long long n, void* stream);
int stx_weighted_lsq_bwd(const float* g_scale, const float* g_shift, const float* mde, const float* disp, const float* conf,
                         const void* stats, float* g_mde, float* g_disp, float* g_conf, int B, long long n, void* stream);
int stx_mirror_detector_fwd(const float* stereo_disp, const float* mono_disp, const float* stereo_conf, const float* mono_conf,
                            float conf_th, float step_gain, float* out, long long n, void* stream);
int stx_mirror_detector_bwd(const float* g_out, const float* stereo_disp, const float* mono_disp, const float* stereo_conf,
                            const float* mono_conf, float conf_th, float step_gain, float* g_stereo_disp, float* g_mono_disp,
                            float* g_stereo_conf, float* g_mono_conf, long long n, void* stream);

/* ---- selfsup_loss.hip: the self-supervised objective (reference loss_functions/), NCHW fp32 ----------------------------------
 * All reductions are deterministic (no float atomics, sums in double); every output element is written once.
 * stx_photo_warp_fwd (photometric_loss.py:5-37): warped [B][C][H][W] = right sampled bilinearly in both directions, zeros
 *   outside, at x = (w - disp) W / (W - 1) - 1/2, y = h H / (H - 1) - 1/2 (the reference's linspace grid under
 *   align_corners=False -- NOT stx_warp_fwd); valid [B][H][W] = the summed weight of the corners inside the image.  H, W >= 2.
 * stx_photo_warp_bwd: gdisp [B][H][W] = -W / (W - 1) sum_c gwarped d warped / d x.  The image gets no gradient.
 * stx_ssim_fwd (:40-77): out [B][C][H][W] = clamp((1 - SSIM) / 2, 0, 1) over window x window boxes of the reflect-padded images;
 *   window odd, 3..11, H and W > window / 2.  The moments are summed in double.
 * stx_ssim_bwd: gx / gy (either may be NULL) from g_out; workspace = stx_ssim_bwd_workspace_floats floats (coefficient maps).
 * stx_photometric_fwd (:80-104): loss [B][1][H][W] = mean_C((w ssim(left, Y) + (1 - w) |left - Y|) valid), window 7,
 *   Y = the warp of right by disp, or right itself when disp is NULL (then enable_mask must be 0); valid only with enable_mask.
 * stx_photometric_bwd: gdisp [B][1][H][W] from gloss, through SSIM, the L1 term and the warp; workspace =
 *   stx_photometric_bwd_workspace_floats floats.  disp must be given.
 * stx_auto_mask_fwd (auto_mask.py:7-17): mask [B][1][H][W] (bytes 0 / 1) = photometric(disp) < photometric(NULL), both without
 *   valid, w = 0.85; denorm != 0 (C = 3) applies x * std + mean of ImageNet to both images first.
 * stx_smoothness_fwd (smoothness_loss.py:5-44): out[0] = mean |dx n| exp(-mean_C |dx img|) + mean |dy n| exp(-mean_C |dy img|),
 *   n = disp / (per-image mean + 1e-7); out[1] = max of img (the caller's range warning, no extra pass); stats = 4 B floats
 *   (2 B doubles: per-image mean and share of the loss) for the backward; workspace = stx_smoothness_workspace_floats floats.
 *   stats and workspace 8-byte aligned.  H, W >= 2.
 * stx_smoothness_bwd: gdisp [B][1][H][W] from the scalar gout (a device pointer), the path through the per-image mean included. */
int stx_photo_warp_fwd(const float* right, const float* disp, float* warped, float* valid, int B, int C, int H, int W, void* stream);
int stx_photo_warp_bwd(const float* gwarped, const float* right, const float* disp, float* gdisp, int B, int C, int H, int W,
                       void* stream);
int stx_ssim_fwd(const float* x, const float* y, float* out, int B, int C, int H, int W, int window, void* stream);
long long stx_ssim_bwd_workspace_floats(int B, int C, int H, int W);
int stx_ssim_bwd(const float* g_out, const float* x, const float* y, float* gx, float* gy, float* workspace, int B, int C, int H, int W,
                 int window, void* stream);
int stx_photometric_fwd(const float* left, const float* right, const float* disp, double ssim_weight, int enable_mask, float* loss,
                        int B, int C, int H, int W, void* stream);
long long stx_photometric_bwd_workspace_floats(int B, int C, int H, int W);
int stx_photometric_bwd(const float* gloss, const float* left, const float* right, const float* disp, double ssim_weight,
                        int enable_mask, float* gdisp, float* workspace, int B, int C, int H, int W, void* stream);
int stx_auto_mask_fwd(const float* left, const float* right, const float* disp, int denorm, unsigned char* mask, int B, int C, int H,
                      int W, void* stream);
long long stx_smoothness_workspace_floats(int B, int H, int W);
int stx_smoothness_fwd(const float* disp, const float* img, float* out, float* stats, float* workspace, int B, int C, int H, int W,
                       void* stream);
int stx_smoothness_bwd(const float* gout, const float* disp, const float* img, const float* stats, float* gdisp, int B, int C, int H,
                       int W, void* stream);

/* ---- sttr_head.hip: STTR's matching head (models/STTR/regression_head.py) on the raw cross-attention attn [N][H][W][W] ---------
 * S = attn (-inf where the right position exceeds the left one) with a dustbin row and column holding *phi (a device scalar),
 * M = W + 1.  mode 1: `iters` log-space Sinkhorn iterations per (n, h) with log mu = log nu = (log_one x W, log_bin) and
 * P = exp(S + u + v + log_2w); mode 0: P = row softmax of S (iters and the three constants unused).  log_one = log(1 / 2W),
 * log_bin = log(W / 2W), log_2w = log(2W) are formed by the CALLER in fp32, the way the reference forms them on the host.
 * One workgroup per (n, h); no float atomics, bitwise reproducible.  Limits: 2 <= W <= 431, 1 <= iters <= 10, fp32 tensors only.
 * Exponents and sums are formed in double; us / vs are doubles.
 * stx_sttr_head_fwd: the fused head, P is never written.  Outputs [N][H][W]: disp = sum over the 3-wide window around the first
 *   arg-max of P_j max(i - j, 0) / norm; norm = the window's sum, forced to 1 where occ_mask (bytes, NULL = none) is set or,
 *   without a mask, where it is below 0.1; occ = 1 - norm; arg = the arg-max index, bit 16 set where norm was forced;
 *   gt_response (with target, both or neither) = P sampled linearly at target between the clamped floor and ceil,
 *   weight_r = target - clamped floor; bin_left = P[:W, W], bin_right = P[W, :W].  us / vs (both or neither, NULL for a plain
 *   forward): mode 1 the scaling vectors u_k, v_k [N][H][iters][M], mode 0 the row max and row sum [N][H][M].
 * stx_sttr_head_bwd: any of the five gradients may be NULL (not all).  g_attn [N][H][W][W] written once per element (exact
 *   zeros at -inf entries); phi_partials [N*H] (doubles) = one partial per matrix, g_phi [1] = their sum in a fixed order.
 * stx_sttr_transport_fwd / _bwd: the dense pair, P and G [N][H][M][M]; the same sweeps. */
int stx_sttr_head_fwd(const float* attn, const float* phi, int mode, int iters, float log_one, float log_bin, float log_2w,
                      const unsigned char* occ_mask, const float* target, float* disp, float* occ, float* norm, int* arg,
                      float* gt_response, float* bin_left, float* bin_right, double* us, double* vs, int N, int H, int W, void* stream);
int stx_sttr_head_bwd(const float* g_disp, const float* g_occ, const float* g_gt, const float* g_bin_left, const float* g_bin_right,
                      const float* attn, const float* phi, int mode, int iters, float log_one, float log_bin, float log_2w,
                      const float* target, const float* disp, const float* norm, const int* arg, const double* us, const double* vs,
                      float* g_attn, double* phi_partials, float* g_phi, int N, int H, int W, void* stream);
int stx_sttr_transport_fwd(const float* attn, const float* phi, int mode, int iters, float log_one, float log_bin, float log_2w,
                           float* P, double* us, double* vs, int N, int H, int W, void* stream);
int stx_sttr_transport_bwd(const float* G, const float* attn, const float* phi, int mode, int iters, float log_one, float log_bin,
                           float log_2w, const double* us, const double* vs, float* g_attn, double* phi_partials, float* g_phi, int N,
                           int H, int W, void* stream);

/* ---- sttr_attention.hip: STTR's attention with relative positional encoding (models/STTR/attention.py), the core between the
 * q/k/v projection and the output projection.  q (already scaled), k, v, o and their gradients [W][B][E][16] -- the memory a
 * linear layer on [W][B][C] leaves; Qr, Kr and their gradients [2W-1][E][16], or all NULL (no positional terms).
 *   S[b][e][w][v] = q[w].k[v] + q[w].Kr[r] + k[v].Qr[r], r = W-1-w+v; causal != 0: -inf where v > w; o = softmax_v(S) v.
 * Limits: head_dim == 16, 2 <= W <= 431, E <= 8, B <= 65535, fp32.  No float atomics, bitwise reproducible.
 * stx_sttr_attn_fwd: raw (NULL or [B][W][W]) = sum_e S in head order, -inf where masked; avg (NULL or [B][W][W]) = mean_e
 *   softmax(S); stats (NULL or [2][B][E][W]) = row max, then row sum: what the backward needs besides o.
 * stx_sttr_attn_bwd: dO or dRaw may be NULL (not both); entries of dRaw at masked positions contribute exactly 0.  nb = the
 *   number of chunks the rows b are split into for the table gradients (1 .. B); scratch holds B * E * W floats and, with
 *   tables, nb * E * W16 * 2 * (W16 + 1) * 256 more, W16 = ceil(W / 16); scratch_floats is its size and is checked. */
int stx_sttr_attn_fwd(const float* q, const float* k, const float* v, const float* Qr, const float* Kr, int causal, float* o,
                      float* raw, float* avg, float* stats, int W, int B, int E, int head_dim, void* stream);
int stx_sttr_attn_bwd(const float* dO, const float* dRaw, const float* q, const float* k, const float* v, const float* Qr,
                      const float* Kr, const float* o, const float* stats, int causal, float* dq, float* dk, float* dv, float* dQr,
                      float* dKr, float* scratch, long long scratch_floats, int nb, int W, int B, int E, int head_dim, void* stream);

/* ---- disp_attention.hip: FoundationStereo's disparity transformer (models/FoundationStereo/submodule.py
 * `CostVolumeDisparityAttention`): `layers` post-norm encoder layers over N sequences of L tokens x C channels, fp32.
 * Sequences are addressed in place: the floats of token t of sequence n start at
 *   (n / hw) * sb + (n % hw) * sp + t * st,  the C channels contiguous
 * (dense [B][D][H][W][C]: N = B H W, L = D, hw = H W, sb = D H W C, sp = C, st = H W C; [N][L][C]: hw = 1, sb = L C, sp = 0,
 * st = C); x, y, gy and gx of a call share one such view; base pointers 16-byte aligned, strides multiples of 4.
 * params / gparams: HOST arrays of 16 * layers device pointers, per layer in state-dict order: q_proj.weight [C][C], q_proj.bias,
 * k_proj.*, v_proj.*, out_proj.*, linear1.weight [F][C], linear1.bias [F], linear2.weight [C][F], linear2.bias [C], norm1.weight,
 * norm1.bias, norm2.weight, norm2.bias.  A NULL entry of gparams is a frozen tensor: its products are skipped.
 * Served (stx_disp_attention_supported returns 1): 1 <= L <= 32; C and F multiples of 4 up to 32; nhead divides C with
 * C / nhead <= 8; 1 <= layers <= 8; also N L C < 2^31.  Anything else is an error and nothing is launched.
 * Layer: Q, K, V = x W^T + b; per head softmax(Q K^T / sqrt(hd)) V; z = x + drop(out_proj(.)); x1 = LayerNorm(z) (eps, biased
 * variance); y = LayerNorm(x1 + drop(linear2(drop(gelu(linear1(x1)))))), exact erf GELU.  pe (NULL or [L][C]) is added to x once in
 * front.  Soft-max, erf and the LayerNorm moments are formed in double and rounded once.
 * Dropout: seed is a DEVICE pointer to one 64-bit integer (NULL or p == 0: nothing is drawn), p the probability as fp32.
 *   Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (n, t >> 2, 4 * layer + site, channel), site 0 behind
 *   out_proj, 1 behind the GELU (F channels), 2 behind linear2; element (layer, site, n, t, channel) is kept iff word (t & 3) of
 *   the result is >= floor((double)p * 2^32); kept values are multiplied by (float)(1 / (1 - (double)p)).  No mask is stored: the
 *   backward draws it again.  stx_disp_attention_masks writes the keep decisions (1 / 0) of a call as bytes
 *   [layers][3][N][L][max(C, F)] (every channel below max(C, F) of every site).
 * stx_disp_attention_fwd: one launch; saved (NULL or [layers][N][L][C]) receives the input of every layer, all the backward needs.
 * stx_disp_attention_bwd: one launch per layer plus a reduction launch, from the last layer down to the lowest one anything is
 *   wanted from; gx may be NULL; gbuf [N][L][C] carries the gradient between layers (may be NULL for one layer); workspace of
 *   stx_disp_attention_bwd_workspace_floats(N, L, C, F) floats (0: not served): one row of parameter gradients per unit of four
 *   consecutive sequences, added in unit order.  No float atomics; the bits do not depend on the grid (switch STX_DA_GRID). */
int stx_disp_attention_supported(int L, int C, int nhead, int F, int layers);
int stx_disp_attention_fwd(const float* x, const float* pe, const float* const* params, float* y, float* saved, const long long* seed,
                           float p, float eps, int N, int L, int C, int nhead, int F, int layers, int hw, long long sb, long long sp,
                           long long st, void* stream);
long long stx_disp_attention_bwd_workspace_floats(int N, int L, int C, int F);
int stx_disp_attention_bwd(const float* gy, const float* saved, const float* const* params, float* const* gparams, float* gx, float* gbuf,
                           float* workspace, long long workspace_floats, const long long* seed, float p, float eps, int N, int L, int C,
                           int nhead, int F, int layers, int hw, long long sb, long long sp, long long st, void* stream);
int stx_disp_attention_masks(const long long* seed, float p, unsigned char* masks, int N, int L, int C, int F, int layers, void* stream);

/* ---- convex_upsample.hip: convex upsampling with the soft-max fused, and the trainer's sequence loss; fp32 tensors -------------
 * RAFT layout (upsample_flow of RAFTStereo / DEFOMStereo, convex_upflow of StereoAnywhere, upsample_disp of SelectiveRAFT):
 *   flow [N][D][H][W], mask [N][9 f f][H][W] (logits, channel (t f + j) f + i), out [N][D][f H][f W]:
 *   out[n][d][f y + j][f x + i] = sum_t softmax_t(mask[n][t][j][i][y][x]) * scale * flow[n][d][y + t/3 - 1][x + t%3 - 1], zero
 *   outside.  f in {2, 4, 8}, mask_channels == 9 f f, D >= 1; anything else is an error and nothing is launched.
 * Pixel layout (IGEV family): disp_low [B][1][h][w], logits [B][9][4h][4w], out [B][4h][4w]:
 *   out[b][Y][X] = sum_t softmax_t(logits[b][t][Y][X]) * scale * disp_low[b][Y/4 + t/3 - 1][X/4 + t%3 - 1].
 * The soft-max (maximum subtracted), the nine-term sums and the gradients are formed in double.  The backward re-forms the
 * soft-max from the logits: nothing but the two inputs is needed.  gflow / gmask (gdisp / glogits): either may be NULL.  The
 * flow's gradient needs a workspace of stx_convex_upsample_bwd_workspace_floats(N, D, H, W) floats (pixel layout: (B, 1, h, w)),
 * 8-byte aligned.  out, g and the pixel layout's logits / glogits must be 16-byte aligned.  No atomics, bitwise reproducible. */
int stx_convex_upsample_fwd(const float* flow, const float* mask, float* out, int N, int D, int H, int W, int mask_channels, int f,
                            float scale, void* stream);
long long stx_convex_upsample_bwd_workspace_floats(int N, int D, int H, int W);
int stx_convex_upsample_bwd(const float* g, const float* flow, const float* mask, float* gflow, float* gmask, float* workspace, int N,
                            int D, int H, int W, int mask_channels, int f, float scale, void* stream);
int stx_softmax_context_upsample_fwd(const float* disp_low, const float* logits, float* out, int B, int h, int w, float scale,
                                     void* stream);
int stx_softmax_context_upsample_bwd(const float* g, const float* disp_low, const float* logits, float* gdisp, float* glogits,
                                     float* workspace, int B, int h, int w, float scale, void* stream);
/* Sequence loss (trainer/trainer_torchrun.py:272-284): loss[0] = sum_k weights[k] * (sum_valid smooth_l1(preds[k] - gt)) /
 *   max(1, #valid), valid = (gt > 0) & (gt < maxdisp - 1), beta = 1; a NaN / inf gt is excluded, never multiplied.  preds is a HOST
 *   array of K device pointers (n floats each), weights a HOST array of K doubles: both are packed by value into the kernel's
 *   arguments.  1 <= K <= stx_sequence_loss_max_predictions(), n < 2^31.  count[0] (device) receives #valid; workspace =
 *   stx_sequence_loss_workspace_floats(n) floats, 8-byte aligned.  No host sync, no float atomics.
 * stx_sequence_loss_bwd: gpreds (HOST array of K device pointers, entries may be NULL) receive
 *   weights[k] * clamp(preds[k] - gt, -1, 1) * gloss[0] / max(1, count[0]), exactly 0 at excluded pixels. */
int stx_sequence_loss_max_predictions(void);
long long stx_sequence_loss_workspace_floats(long long n);
int stx_sequence_loss_fwd(const float* const* preds, const double* weights, int K, const float* gt, float maxdisp, float* loss,
                          int* count, float* workspace, long long n, void* stream);
int stx_sequence_loss_bwd(const float* gloss, const float* const* preds, const double* weights, int K, const float* gt, float maxdisp,
                          const int* count, float* const* gpreds, long long n, void* stream);

/* ---- monster.hip: MonSter's mono / stereo mutual refinement (models/MonSter/monster.py:456-494, warp.py), NCHW fp32 -----------
 * The sample of disp_warp: ix = (x - d) W / (W - 1) - 1/2, iy = y H / (H - 1) - 1/2 (formed in double), bilinear in both
 * directions; zeros_pad == 0: padding 'border' (ix clipped to [0, W - 1], iy to [0, H - 1]; a clipped ix has no gradient to d),
 * zeros_pad != 0: padding 'zeros'.  H, W >= 2, B C H W < 2^31, B <= 65535.  No float atomics, no memset, bitwise reproducible.
 * stx_monster_flaw_fwd: out_a [B][C][H][W] = right sampled with disp_a [B][H][W], minus left (left NULL: the sample itself);
 *   out_b the same with disp_b (both or neither); valid (NULL or [B][H][W]) = the validity map of disp_a: 1 under 'border', under
 *   'zeros' 0 where the summed weight of the corners inside the image is below 0.9999, else 1.  One launch.
 * stx_monster_flaw_bwd: from g_a / g_b (either may be NULL: no contribution), any of g_left = -(g_a + g_b), g_right (gathered:
 *   every element written once, a's rows before b's, ascending output row, ascending output column; W <= 2048),
 *   g_disp_a / g_disp_b [B][H][W] = -W / (W - 1) sum_c g d out / d ix (NULL = skipped).  At most two launches.
 * stx_monster_scale_shift (monster.py:31-66): per image b of n elements, thr = the k-th smallest mono value (0-based, exact);
 *   under mask (bytes; NULL: (gt > 0) & (mono > 1e-2) & (mono > thr)) the sums S_mm, S_m, N, S_mg, S_g in double and
 *   out[b] = (scale, shift) = the solution of (X^T X + 1e-6 I) p = X^T y in double, rounded once; an empty mask gives (0, 0).
 *   stats [B][8] doubles: the five sums, thr, k, 0.  1 <= n < 2^24, 0 <= k < n.  One workgroup per image, no host sync.
 * stx_monster_apply_scale_shift: out[b] = scale_b x[b] + shift_b (with_shift == 0: scale_b x[b], the backward). */
int stx_monster_flaw_fwd(const float* left, const float* right, const float* disp_a, const float* disp_b, int zeros_pad, float* out_a,
                         float* out_b, float* valid, int B, int C, int H, int W, void* stream);
int stx_monster_flaw_bwd(const float* g_a, const float* g_b, const float* right, const float* disp_a, const float* disp_b, int zeros_pad,
                         float* g_left, float* g_right, float* g_disp_a, float* g_disp_b, int B, int C, int H, int W, void* stream);
int stx_monster_scale_shift(const float* mono, const float* gt, const unsigned char* mask, long long k, float* out, void* stats, int B,
                            long long n, void* stream);
int stx_monster_apply_scale_shift(const float* x, const float* scale_shift, int with_shift, float* out, int B, long long n,
                                  void* stream);

/* ---- instnorm.hip: instance normalisation + activation (+ residual tail), fp32 -------------------------------------------------
 * nn.InstanceNorm2d / 3d with affine=False, track_running_stats=False, biased variance (the reference's IGEV BasicConv_IN /
 * Conv2x_IN and the RAFT-family ResidualBlock).  `planes` = B C planes of S = H W or D H W floats each; layout 0 = every plane one
 * contiguous run (NCHW / NCDHW), the only layout the kernels serve (a channels-last tensor goes through one copy in the binding).
 *   xhat = (x - mean) / sqrt(var + eps);  y = act(xhat), or with skip (same shape): y = relu(skip + act(xhat)).
 *   act: 0 none, 1 ReLU, 3 LeakyReLU(0.01).  S >= 2, S < 2^31.  x, skip, y, gy, gx, gskip 16-byte aligned.
 * A plane is cut into chunks by a rule of (planes, S) alone: stx_instnorm_plan returns the chunks per plane and the path
 *   (0: one chunk per plane, one launch; 1: two launches, per-chunk partial sums in the workspace, then apply).
 *   stx_instnorm_ws_bytes: bytes of that workspace (8-byte aligned; 0 on path 0, -1 for arguments the kernels refuse).
 * stx_instnorm_fwd: stats (NULL or [planes][2] DOUBLES: mean, 1 / sqrt(var + eps)) is what the backward needs besides x and skip.
 *   The sums, the moments and the expression above are formed in double from the fp32 input and rounded once.
 * stx_instnorm_bwd: gx = rstd (g' - mean(g') - xhat mean(g' xhat)), g' = gy [y > 0 with skip] act'(xhat); gskip = gy [y > 0].
 *   Either may be NULL (gskip needs skip).  xhat and the masks are re-formed: y is not needed.  ReLU passes where its input is
 *   > 0, LeakyReLU has slope 0.01 where xhat <= 0.  No float atomics: bitwise reproducible. */
int stx_instnorm_plan(long long planes, long long S, int layout, int* chunks, int* path);
long long stx_instnorm_ws_bytes(long long planes, long long S, int layout);
int stx_instnorm_fwd(const float* x, const float* skip, float* y, void* stats, void* workspace, long long planes, long long S,
                     int layout, int act, float eps, void* stream);
int stx_instnorm_bwd(const float* gy, const float* x, const float* skip, const void* stats, float* gx, float* gskip, void* workspace,
                     long long planes, long long S, int layout, int act, void* stream);

#ifdef __cplusplus
}
#endif
#endif
