/*
 * atvsnet_hip.h -- C-ABI of the MI355X (gfx950) kernels for the A-TVSNet
 * two-view cost-volume inference path.
 *
 * This is the drop-in boundary: plain pointers, sizes and
 * scalars, no framework types.  Every pointer is a DEVICE pointer to float32
 * data unless stated otherwise; tensors are dense, row-major, channel-last
 * (the reference's NDHWC / NHWC), batch size 1 (FLAGS.batch_size, example.py:45).
 * The caller owns every buffer (outputs and workspaces included); kernels never
 * allocate.  Calls are asynchronous on `stream` (a hipStream_t; NULL = default
 * stream), re-entrant per stream, hold no global state, and return ATVS_OK or a
 * negative error code (no exceptions cross the ABI).
 *
 * Each entry point names the reference TensorFlow op chain it replaces
 * (paths relative to the reference repository root).
 */
#ifndef ATVSNET_HIP_H
#define ATVSNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* atvs_stream_t; /* hipStream_t */

enum {
  ATVS_OK = 0,
  ATVS_ERR_NULL = -1,   /* a required pointer is NULL */
  ATVS_ERR_SHAPE = -2,  /* inconsistent or unsupported sizes */
  ATVS_ERR_ARG = -3,    /* bad enum / flag value */
  ATVS_ERR_LAUNCH = -4  /* the HIP runtime rejected the launch */
};

/* ABI version of this header (bumped on any signature change).  atvs_abi_version() returns the value the library
 * was compiled with; the loader (a-tvsnet_amd/_lib.py) refuses a library whose version differs from this header's. */
#define ATVS_ABI_VERSION 66
int atvs_abi_version(void);
/* "gfx950" -- the only code object in the library. */
const char* atvs_target_arch(void);

/* ------------------------------------------------------------------------- *
 * Geometry  (atvsnet/homography_warping.py)
 * ------------------------------------------------------------------------- */

/* get_homographies, homography_warping.py:179-227.
 * left_cam/right_cam: (2,4,4) [extrinsic; K + depth range].  depth_start,
 * depth_interval: 1 float each.  homographies out: (depth_num,3,3). */
int atvs_get_homographies(const float* left_cam, const float* right_cam, const float* depth_start,
                          const float* depth_interval, float* homographies, int depth_num,
                          int inverse_depth, atvs_stream_t stream);

/* D x homography_warping(bilinear) + tf.stack, with the caller's epilogue fused:
 * homography_warping.py:230-271 + :31-104, unrolled over d at model.py:190-194,
 * 272-279, 292-297.
 *   src (h,w,C); homographies (D,3,3); out (D,h,w,ld_out) written at channels
 *   [c_off, c_off+C) (mode 2: [c_off, c_off+rep)); mask_out (D,h,w) or NULL.
 *   mode 0: warp.   mode 1: |warp - ref| * mask, ref (h,w,C) (photo volume).
 *   mode 2: C == 1; (|warp - delta_d| / interval / D) * mask replicated to `rep`
 *           channels (geo view volume, reference quirk: 16 identical channels).
 *   mode 3: nearest-neighbour warp (homography_warping.py:45-56: tf.round half-to-even,
 *           out-of-range pixels read source pixel (0,0) and are NOT zeroed; mask_out tells).
 *   planar != 0 (mode 0 or 1, C in {16, 32, 64}, ld_out == C, c_off == 0): out is written chunk-planar,
 *           [C/8] planes of [D][h][w][8], `planar` floats apart (>= D*h*w*8; pad it so that the planes do not start
 *           on the same HBM channel) -- the layout atvs_conv_xw_f32 / _xb_f32 read with x_planar (dense 32-byte
 *           voxels per 8-channel chunk); same values, another place.  The pad between the planes is never written.
 *   pieces != 0 (with planar): every value is written as its two fp16 pieces, h0 = fp16(x), h1 = fp16((x - h0) * 2048) -- the
 *           operand split of the split-operand convolutions, done once by the producer: a chunk plane then holds
 *           [2 pieces][D][h][w][8 fp16] (the same D*h*w*32 bytes), which atvs_conv_xb_f32 reads with x_pieces and stages
 *           by LDS-DMA. */
int atvs_warp_planes(const float* src, const float* homographies, const float* ref,
                     const float* depth_start, const float* depth_interval, float* out, float* mask_out,
                     int D, int h, int w, int C, int ld_out, int c_off, int mode, int rep, long planar, int pieces,
                     atvs_stream_t stream);

/* build_cost_volume, model.py:157-200: tf.tile(ref) ++ stack_d(warp_d(view)) ->
 * cost_volume (D,h,w,2C).  C % 4 == 0. */
int atvs_build_cost_volume(const float* ref_feature, const float* view_feature, const float* homographies,
                           float* cost_volume, int D, int h, int w, int C, atvs_stream_t stream);

/* tf.tile(tf.expand_dims(x,1),[1,D,1,1,1]) into a channel slice: model.py:311,316,329-330. */
int atvs_tile_planes(const float* src, float* out, int D, int h, int w, int C, int ld_out, int c_off,
                     atvs_stream_t stream);

/* cost_volume_geo_ref, model.py:289-290: |depth_ref - delta_d| / interval / D into channel c_off. */
int atvs_geo_ref_planes(const float* depth_ref, const float* depth_start, const float* depth_interval,
                        float* out, int D, int h, int w, int ld_out, int c_off, atvs_stream_t stream);
/* geo_ref and geo_view of the refinement (model.py:285-300) in one launch: out (D,h,w,ld)[..., c_off] = atvs_geo_ref_planes,
 * [..., c_off + 1 .. c_off + rep] = atvs_warp_planes(mode 2, rep) of the one-channel map view_depth (h,w) -- the same values. */
int atvs_geo_volume(const float* depth_ref, const float* view_depth, const float* homographies, const float* depth_start,
                    const float* depth_interval, float* out, int D, int h, int w, int ld_out, int c_off, int rep,
                    atvs_stream_t stream);

/* get_visual_hull with view_num = 2, homography_warping.py:329-387: out (D,h,w).
 * view_depth_in_ref = transform_depth(view depth, view_cam, ref_cam). */
int atvs_visual_hull(const float* ref_depth, const float* view_depth_in_ref, const float* homographies,
                     const float* depth_start, const float* depth_interval, float* out, int D, int h, int w,
                     int inverse_depth, atvs_stream_t stream);

/* homography_warping_by_depth, homography_warping.py:108-176.  method 0 bilinear,
 * 1 nearest.  mask_out (h,w) or NULL.  pose_ws: 12 floats of scratch. */
int atvs_warp_by_depth(const float* src, const float* left_cam, const float* right_cam, const float* depth,
                       float* out, float* mask_out, float* pose_ws, int h, int w, int C, int method,
                       int inverse_depth, atvs_stream_t stream);

/* |homography_warping_by_depth(src) - ref| * mask into channels [c_off, c_off + C) of out (h,w,ld_out): photo_err / geo_err of the
 * refinement (model.py:309-316) in one launch; the operations and order of atvs_warp_by_depth + atvs_absdiff_mask.
 * copy_ref != 0: ref itself is written to the C channels behind the error map (the tiled map that follows it, :329-334). */
int atvs_warp_by_depth_err(const float* src, const float* ref, const float* left_cam, const float* right_cam,
                           const float* depth, float* out, int ld_out, int c_off, int h, int w, int C, int method,
                           int inverse_depth, int copy_ref, atvs_stream_t stream);

/* interpolate, homography_warping.py:31-104, with caller-supplied coordinates: src (h,w,C), x / y (n) in the
 * reference's texture coordinates (pixel centres at +0.5), out (n,C), mask_out (n) 1.f / 0.f or NULL.  method 0
 * bilinear (invalid points give 0), 1 nearest (tf.round; invalid points read pixel (0,0), not masked). */
int atvs_interpolate(const float* src, const float* x, const float* y, float* out, float* mask_out, long n,
                     int h, int w, int C, int method, atvs_stream_t stream);

/* get_pixel_grids, homography_warping.py:8-17: out (3*h*w) = [x + 0.5 | y + 0.5 | 1], row-major pixels. */
int atvs_pixel_grids(float* out, int h, int w, atvs_stream_t stream);

/* transform_depth, homography_warping.py:275-326.  ws14: 14 floats of scratch. */
int atvs_transform_depth(const float* depth, const float* left_cam, const float* right_cam, float* out,
                         float* ws14, int h, int w, int inverse_depth, atvs_stream_t stream);
/* n <= 16 maps of one size in one launch (a map per workgroup; h * w <= 32,768: atvs_transform_depth_batch_supported): the values of n
 * calls of atvs_transform_depth (the refinement transforms every source view's depth map twice, model.py:289,321-324).  The four
 * arguments are HOST arrays of n device pointers. */
int atvs_transform_depth_batch_supported(int h, int w);
int atvs_transform_depth_batch(const float* const* depth, const float* const* left_cam, const float* const* right_cam,
                               float* const* out, int n, int h, int w, int inverse_depth, atvs_stream_t stream);

/* tf.abs(a - b) * tile(mask): photo_err / geo_err, model.py:310,315.
 * a, b, out (npix, C); mask (npix). */
int atvs_absdiff_mask(const float* a, const float* b, const float* mask, float* out, int npix, int C,
                      atvs_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Soft-argmin  (atvsnet/model.py)
 * ------------------------------------------------------------------------- */

/* prob2depth, model.py:80-109: cost (groups,D,h,w) -> depth (groups,h,w); the volumes of a launch share the depth sweep. */
int atvs_softargmin(const float* cost, const float* depth_start, const float* depth_interval,
                    float* depth_out, int groups, int D, int h, int w, atvs_stream_t stream);

/* upsample_prob_vol + prob2depth, model.py:68-76,121-127: cost (D,h,w) ->
 * depth (h*up, w*up) without materialising the upsampled volume. */
int atvs_upsample_softargmin(const float* cost, const float* depth_start, const float* depth_interval,
                             float* depth_up_out, int D, int h, int w, int up_scale, atvs_stream_t stream);

/* get_propability_map (model.py:13-65) as used by prob2depth / prob2depth_upsample(out_prob_map=True)
 * (:104-107, :122-125; the ETH3D driver eval_pointcloud.py:232,269): per pixel the sum of the probabilities of
 * the four depth planes around the estimated depth, l0 = clip(floor(d)), l1 = clip(l0-1), r0 = clip(ceil(d)),
 * r1 = clip(r0+1), d = (depth - depth_start) / depth_interval.  vol (D,h,w); depth_map, prob_out
 * (h*up_scale, w*up_scale).  softmax != 0: vol is the pre-softmax cost and P = softmax(-vol) is evaluated on
 * the fly; up_scale > 1: vol is read through the align_corners bilinear interpolation of upsample_prob_vol
 * (:66-75) -- neither the probability volume nor its upsampled copy is materialised. */
int atvs_probability_map(const float* vol, const float* depth_map, const float* depth_start,
                         const float* depth_interval, float* prob_out, int D, int h, int w, int up_scale, int softmax,
                         atvs_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Convolutions  (cnn_wrapper/network.py)
 * ------------------------------------------------------------------------- */

/* Sizes of the packed weights / group table for `ntaps` taps (see atvs_conv_pack).
 * vec = 4 when Cin % 4 == 0 else 1; ksteps = ceil(ntaps*Cin/vec / 4); ntiles = Cout
 * rounded up to 16, 32, 64 or 128, over 16.  Host function, no GPU work. */
int atvs_conv_pack_size(int ntaps, int Cin, int Cout, int* vec, int* ksteps, int* ntiles,
                        long* packed_floats, long* table_ints);

/* HOST function (plain CPU loops, host pointers): arrange a TF-layout kernel for
 * atvs_conv_mfma_f32.  w: [n_w_taps][Cin][Cout] (w_transposed = 0, tf.layers.conv2d/3d
 * kernels [k.., Cin, Cout]) or [n_w_taps][Cout][Cin] (w_transposed = 1,
 * conv3d_transpose kernels [k.., Cout, Cin]).  taps: ntaps x 4 int32 =
 * (index of the tap in w, dz, dy, dx), (dz,dy,dx) = input offset relative to
 * output_index * in_stride (SAME / explicit padding and dilation folded in; the 8
 * parity classes of a stride-2 transposed convolution are 8 tap lists).
 * The caller uploads `packed` and `table` to the device. */
int atvs_conv_pack(const float* w, int w_transposed, const int32_t* taps, int ntaps, int Cin, int Cout,
                   float* packed, int32_t* table);

/* Workgroups a launch with M = Do*Ho*Wo output voxels and `tile_m` uses
 * (= rows of stats_partial): ceil(M / (64 * tile_m)). */
long atvs_conv_num_blocks(long M, int tile_m);

/* tf.layers.conv2d / conv3d / conv3d_transpose (one parity class per call),
 * slim.conv2d, tf.nn.conv3d + bias_add + residual add + relu, on the fp32 matrix
 * cores: network.py:141-215, 282-351, 510-602.
 *   x (Di,Hi,Wi,Cin) (2-D: Di = 1); y rows of width ldy, channels [y_coff, y_coff+Cout)
 *   of the full output tensor (Dy,Hy,Wy); this launch writes output voxels
 *   o*out_stride + off for o in the logical grid (Do,Ho,Wo) and reads inputs at
 *   o*in_stride + tap offset.  bias (Cout) / residual (same addressing as y,
 *   y_coff must be 0) may be NULL.  relu != 0 applies max(.,0) last.
 *   plane_bias: NULL, or (Ho,Wo,3*Cout): the contribution of input channels that are
 *   constant along depth (the tf.tile'd halves of model.py:186,311,316,329-330), i.e. the
 *   2-D convolution of those channels with the kd-summed kernel, for the three sets of
 *   in-range kd taps [kd=0 missing | all | kd=2 missing]; added per output voxel according
 *   to its plane (pad_z = z padding before).  3x3x3 kernels, out_stride 1 only.
 *   stats_partial: NULL, or [atvs_conv_num_blocks][2][16*ntiles] doubles receiving
 *   per-workgroup (sum, sum of squares) of the values written, per channel, for
 *   training-mode batch norm (network.py:206-212).  tile_m in {1,2,4,8},
 *   tile_m * ntiles <= 16.
 *   groups >= 1: x, y, residual and plane_bias are `groups` independent samples stacked on a leading axis (one
 *   network call each in the reference); a workgroup never spans samples and stats_partial has
 *   groups * atvs_conv_num_blocks rows, sample-major (atvs_bn_finalize reduces them per sample). */
int atvs_conv_mfma_f32(const float* x, const float* packed_w, const int32_t* group_table, const float* bias,
                       const float* residual, const float* plane_bias, int pad_z, float* y,
                       double* stats_partial, int groups, int Di, int Hi, int Wi,
                       int Cin, int Do, int Ho, int Wo, int in_stride, int Dy, int Hy, int Wy,
                       int out_stride, int off_z, int off_y, int off_x, int ldy, int y_coff, int Cout,
                       int ntaps, int tile_m, int relu, atvs_stream_t stream);

/* LDS-tiled variant of the same convolution for halo-1 stencils: 3-D, input step 1, every
 * tap offset in [-1,1]^3 (3x3x3 stride-1 SAME convolutions; each parity class of the
 * stride-2 transposed convolution).  A workgroup computes a 4 x tile_y x 16 block of the
 * logical output grid (= the input grid D,H,W) from an input halo tile staged once in LDS.
 * atvs_conv_tiled_pack_size / _pack are the HOST packing functions for it (same inputs
 * as atvs_conv_pack; the table depends on tile_y in {4, 8}).  The grid is persistent
 * (atvs_conv_tiled_num_blocks workgroups sweep the tiles); stats_partial has that many rows of
 * 16*ntiles doubles x 2 (one per workgroup).  Small volumes deal the 16-channel output tiles of a
 * spatial tile to several workgroups (atvs_conv_tiled_grid reports nsplit): each then fills its own
 * columns of its row and zeros in the others.  Launches whose per-workgroup
 * width is 128 channels produce no statistics (atvs_conv_tiled_has_stats == 0: pass NULL and
 * use atvs_channel_stats on the output).
 * Fused stride-2 transposed convolution (class_cout != 0): the 8 output parity classes of
 * conv3d_transpose(3, stride 2, SAME) are computed from ONE staged tile -- the GEMM's N axis is
 * (class, channel): Cout = n_classes * class_cout "virtual" channels over the 8 taps
 * {-1,0}^3 with the dense virtual kernel Wv[off][ci][(class, co)] = W[k(off, class)] or 0; virtual
 * channel (c, co) of grid voxel j is written to output voxel 2j + parity(class_base + c); the
 * statistics columns (c, co) fold onto co in atvs_bn_finalize(fold = n_classes).
 * x-pair form (xpair != 0, Cout == 8 only): the 16 GEMM rows are (x parity, channel) and a tile column
 * is the voxel pair (2i, 2i+1), so no row of the MFMA tile is padding; the packed kernel is the dense
 * virtual kernel Wv[(kd,kh,ox)][ci][(jx,co)] = W[kd][kh][ox-jx+1] (or 0) over the 36 taps
 * ox in -1..2 (pack with xpair = 1 and 16 output channels); tile_y = 4 for 16-channel chunks.
 * In-launch finalize (fin_counter != NULL): the last workgroup to arrive (one agent-scope atomic ticket on
 * *fin_counter, which must be zero before the layer's first launch and is left at zero) reduces the
 * fin_rows rows of fin_stats (the layer's whole statistics buffer; fin_arrivals = workgroups of all the
 * layer's launches) into fin_params = (3, fin_channels) floats (mean, rsqrt(var + fin_eps), 0), exactly
 * what atvs_bn_finalize(beta = NULL) would write -- no separate finalize launch.  fin_channels <= 64.
 * `table` (atvs_conv_tiled_pack): per K step the 4 LDS offsets of its (tap, channel group) entries, then per
 * K step a bit mask of the 16-channel output tiles whose packed weights are not all zero -- the kernel skips
 * the others (the structural zeros of the fused transposed convolution: 44-58 % of its tile-steps). */
int atvs_conv_tiled_pack_size(int ntaps, int Cin, int Cout, int* nchunk, int* chunk_pad, int* ksteps_per_chunk,
                              int* ntiles, long* packed_floats, long* table_ints);
int atvs_conv_tiled_pack(const float* w, int w_transposed, const int32_t* taps, int ntaps, int Cin, int Cout,
                         int tile_y, int xpair, float* packed, int32_t* table);
/* groups >= 1 independent samples stacked on the leading axis of x / y / residual / plane_bias: the persistent grid is
 * shared out among the samples (atvs_conv_tiled_num_blocks / _grid return the workgroups PER SAMPLE; stats_partial has
 * groups times that many rows, sample-major); the in-launch finalize needs groups == 1. */
long atvs_conv_tiled_num_blocks(int Do, int Ho, int Wo, int tile_y, int Cin, int Cout, int xpair, int groups);
long atvs_conv_tiled_grid(int Do, int Ho, int Wo, int tile_y, int Cin, int Cout, int xpair, int groups, int* nsplit_out);
int atvs_conv_tiled_has_stats(int Do, int Ho, int Wo, int tile_y, int Cin, int Cout, int groups);
int atvs_conv_tiled_f32(const float* x, const float* packed_w, const int32_t* table, const float* bias,
                        const float* residual, const float* plane_bias, float* y, double* stats_partial,
                        int groups, int D, int H, int W, int Cin,
                        int Dy, int Hy, int Wy, int out_stride, int off_z, int off_y, int off_x, int ldy,
                        int y_coff, int Cout, int ntaps, int tile_y, int relu, int class_cout, int class_base,
                        int xpair, uint32_t* fin_counter, float* fin_params, double* fin_stats, int fin_rows,
                        int fin_arrivals, int fin_channels, int fin_fold, long fin_count, float fin_eps,
                        atvs_stream_t stream);

/* conv / conv_bn(3, 8, 1) on a full-resolution volume -- 3x3x3 SAME stride-1 convolution to EIGHT output
 * channels (conv_b*_0_1, global_refine_3dconv0_1, the refinement stems; cnn_wrapper/atvsnet.py, layer code
 * cnn_wrapper/network.py:165-215), Cin % 8 == 0.  x-pair form (two x-adjacent voxels fill the 16 MFMA rows),
 * ONE workgroup per CU with the whole register file and LDS.  Two kernels share the contract: conv_xb.hip (split fp16
 * operands on the 16-bit matrix cores: the product's kernel) and conv_xw.hip (fp32 matrix cores, Winograd F(2,3) along y:
 * the A/B form, ops.configure(split16=False)).
 *   atvs_conv_x{w,b}_pack_size / _pack  HOST: pack the TF kernel [3,3,3,Cin,8] (upload the result)
 *   atvs_conv_xpair_grid                   workgroups of a launch PER SAMPLE = rows of stats_partial per sample ([2][16] doubles
 *                                       each, columns 0..7 = channels, the layout atvs_bn_finalize takes with cpad 16)
 *   atvs_conv_x{w,b}_f32                y (D,H,W,ldy)[..., y_coff + co] = conv(x) (+ bias, + plane_bias (H,W,24), ReLU)
 * Sibling: the U-Nets feed the same tensor to conv_b*_0_1 (8 channels, stride 1) and to the encoder branch
 * conv_b*_1_0 (16 channels, stride 2; cnn_wrapper/atvsnet.py StackedUNet, CostVolRefineNet 0_1 / 1_0).  With
 * packed_w2 != NULL (atvs_conv_x{w,b}_pack_sibling of the TF kernel [3,3,3,Cin,16]) the launch also writes
 * y2 (ceil(D/2), ceil(H/2), ceil(W/2), ldy2)[..., y_coff2 + co] = that stride-2 SAME convolution (+ plane_bias2
 * (Ho2, Wo2, 48)) from the tile already staged in LDS, and its moments into stats_partial2 (same rows).
 * groups >= 1 independent samples stacked on the leading axis of every tensor.
 * Prologue (normalise-on-load / add-on-load): with in_params != NULL the convolution's input is relu?((x - mean) * rstd +
 * beta) per sample, parameters (groups, 3, Cin) -- the producer's training-mode batch norm, network.py:206-212 -- and with
 * x2 != NULL the SUM of two such terms (in_params2 for x2; either parameter block may be NULL = that term as is): the
 * U-Net's skip add (network.py:695-697) formed while the halo is staged.  Out-of-volume taps stay zero.  Built for the
 * shapes the path has: in_params with Cin % 16 == 0 and a sibling; x2 with a sibling and Cin % 16 == 8 (conv_xw) /
 * Cin == 8 (conv_xb) -- else ATVS_ERR_ARG / ATVS_ERR_SHAPE. */
long atvs_conv_xpair_grid(int D, int H, int W, int groups);

/* The fp32 form, conv_xw.hip: x-pair rows x minimal filtering F(2,3) along y -- two output rows from 4 products per
 * (kd, x offset, channel) instead of 6.  The filter transform
 * U = [g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2] is applied by the HOST packer in double; the input transform
 * [d0-d2, d1+d2, d2-d1, d1-d3] in registers from the raw rows staged in LDS (8-channel chunks, double-buffered image).
 * Results differ from the direct sum by fp32 rounding only (one 32 -> 8 layer: 7.7e-7 of the output maximum).
 * x_planar != 0 (no prologue): x is chunk-planar per sample, Cin/8 planes of [D][H][W][8] x_planar floats apart, as
 * atvs_warp_planes writes it with the same `planar` (sample stride = x_planar * Cin / 8). */
int atvs_conv_xw_pack_size(int Cin, long* packed_floats);
int atvs_conv_xw_pack(const float* w, int Cin, float* packed);
int atvs_conv_xw_pack_sibling_size(int Cin, long* packed_floats);
int atvs_conv_xw_pack_sibling(const float* w2, int Cin, float* packed);
int atvs_conv_xw_f32(const float* x, const float* packed_w, const float* bias, const float* plane_bias, float* y,
                     double* stats_partial, int groups, int D, int H, int W, int Cin, int ldy, int y_coff, int relu,
                     const float* packed_w2, const float* plane_bias2, float* y2, double* stats_partial2, int ldy2,
                     int y_coff2, const float* x2, const float* in_params, const float* in_params2, int in_relu,
                     int in_relu2, long x_planar, atvs_stream_t stream);

/* The same layers (same contract as atvs_conv_xw_f32, x_planar included) on the 16-bit matrix cores with SPLIT operands
 * (conv_xb.hip): every fp32 operand = TWO fp16 pieces, x = h0 + h1 / 2048 (h1 = fp16((x - h0) * 2048)), the three products
 * h0 g0 + (h0 g1 + h1 g0) / 2048 accumulated in fp32 by v_mfma_f32_16x16x32_f16 -- fp32-class results (22 significant bits per
 * operand; |x| or |w| beyond 65504 gives inf / NaN, the packers return ATVS_ERR_ARG for such weights), 9 K steps of 16-cycle
 * instructions per (8-channel chunk, kd, kh) row instead of 36 fp32 steps of 32 cycles.  Weights: atvs_conv_xb_pack /
 * _pack_sibling (HOST; sizes in BYTES).  Beyond atvs_conv_xw_f32: x_planar may come with in_params (a pending batch norm
 * over a chunk-planar input: the refinement's concat; not with x2); y_group_stride != 0 = floats between the samples of y
 * (>= D*H*W*ldy; 0 = dense): with ldy = 8 the output lands in one 8-channel plane of each sample's chunk-planar buffer.
 * x2 (two sources) needs Cin == 8; a prologue needs Cin <= 160 (its parameters live in LDS).
 * x_pieces != 0 (with x_planar, no prologue): the chunk planes hold the two fp16 pieces of every value, [2][D][H][W][8 fp16] as
 * atvs_warp_planes(pieces) writes them; the launch then only moves them into LDS (LDS-DMA), the same products follow. */
int atvs_conv_xb_pack_size(int Cin, long* packed_bytes);
int atvs_conv_xb_pack(const float* w, int Cin, unsigned char* packed);
int atvs_conv_xb_pack_sibling_size(int Cin, long* packed_bytes);
int atvs_conv_xb_pack_sibling(const float* w2, int Cin, unsigned char* packed);
int atvs_conv_xb_f32(const float* x, const unsigned char* packed_w, const float* bias, const float* plane_bias, float* y,
                     double* stats_partial, int groups, int D, int H, int W, int Cin, int ldy, int y_coff, int relu,
                     const unsigned char* packed_w2, const float* plane_bias2, float* y2, double* stats_partial2, int ldy2,
                     int y_coff2, const float* x2, const float* in_params, const float* in_params2, int in_relu,
                     int in_relu2, long x_planar, long y_group_stride, int x_pieces, atvs_stream_t stream);

/* 3x3 stride-1 SAME 2-D convolution (dilation 1, 2 or 4) of wide feature maps, LDS-tiled (conv2d_lds.hip): the
 * heavy layers of the feature towers -- the bottlenecks' conv2 (slim.conv2d, network.py:585-587), conv0_1 / conv0_2 /
 * fusion0 (tf.layers.conv2d, network.py:198-200; cnn_wrapper/atvsnet.py:254-292).  x (G,H,W,Cin): G independent
 * images (one tower call each in the reference), Cin % 16 == 0, Cout in {32, 64, 128} (dilation 2 / 4: Cout 128).
 *   atvs_conv2d_lds_supported   1 if (Cin, Cout, dilation) is served by this kernel
 *   atvs_conv2d_lds_pack_size / _pack   HOST: pack the TF kernel [3,3,Cin,Cout] (upload the result)
 *   atvs_conv2d_lds_rows        workgroups per image = rows per image of stats_partial ([2][Cout] doubles each)
 *   atvs_conv2d_lds_f32         y (G,H,W,ldy)[..., y_coff + co] = conv(x) (+ bias, + residual, ReLU); in_params
 *                               (G,3,Cin) != NULL: x is a raw convolution output and its batch norm (mean, rstd,
 *                               beta per image) [+ ReLU if in_relu] is applied while the tile is staged
 *                               (normalise-on-load; the SAME padding stays zero). */
int atvs_conv2d_lds_supported(int Cin, int Cout, int dilation);
int atvs_conv2d_lds_pack_size(int Cin, int Cout, long* packed_floats);
int atvs_conv2d_lds_pack(const float* w, int Cin, int Cout, float* packed);
long atvs_conv2d_lds_rows(int H, int W, int Cout);
int atvs_conv2d_lds_f32(const float* x, const float* packed_w, const float* bias, const float* residual,
                        const float* in_params, int in_relu, float* y, double* stats_partial, int G, int H, int W,
                        int Cin, int Cout, int dilation, int ldy, int y_coff, int relu, atvs_stream_t stream);

/* The same layers (same contract, shapes with Cin % 32 == 0, statistics rows = atvs_conv2d_lds_rows) with SPLIT operands
 * (conv2d_b.hip: every fp32 operand = two fp16 pieces, three products, fp32 accumulation on v_mfma_f32_16x16x32_f16; the
 * arithmetic of atvs_conv_c16b_f32).  Weights: atvs_conv2d_b_pack (HOST; size in BYTES; ATVS_ERR_ARG for a weight beyond
 * fp16's range). */
int atvs_conv2d_b_pack_size(int Cin, int Cout, long* packed_bytes);
int atvs_conv2d_b_pack(const float* w, int Cin, int Cout, unsigned char* packed);
int atvs_conv2d_b_f32(const float* x, const unsigned char* packed_w, const float* bias, const float* residual,
                      const float* in_params, int in_relu, float* y, double* stats_partial, int G, int H, int W, int Cin,
                      int Cout, int dilation, int ldy, int y_coff, int relu, atvs_stream_t stream);

/* A residual unit's conv2 AND conv3 in one launch (reference cnn_wrapper/network.py:585-601; conv2d_b.hip, TAIL form):
 *   y = conv3_1x1(relu(conv2_3x3_dil(x) + b2)) + b3 + residual
 * x (G,H,W,C) = the unit's conv1 output; packed_w2 = atvs_conv2d_b_pack of [3][3][C][C], packed_w3 = atvs_conv1x1_b_pack of
 * [C][C]; residual (G,H,W,C) = the shortcut or NULL; stats_partial: moments of y (rows: atvs_conv2d_lds_rows) or NULL.  r2 crosses
 * the wavefronts through LDS as fp16 pieces.  For the 128-channel dilated units (atvs_conv2d_b_tail_supported: C = 128, dilation
 * 2 / 4), whose conv1 halo does not fit the fully fused unit (atvs_bottleneck_b_f32).  Bit for bit atvs_conv2d_b_f32 followed by
 * atvs_conv1x1_b_f32. */
int atvs_conv2d_b_tail_supported(int C, int dilation);
int atvs_conv2d_b_tail_f32(const float* x, const unsigned char* packed_w2, const float* b2, const unsigned char* packed_w3,
                           const float* b3, const float* residual, float* y, double* stats_partial, int G, int H, int W, int C,
                           int dilation, atvs_stream_t stream);

/* The strided conv2 of a residual unit's first block (reference cnn_wrapper/network.py:588-595: explicit symmetric padding 1 +
 * VALID, stride 2 -- taps centred on input pixel 2 i, quirk C17) on the split-operand kernel (conv2d_b.hip, STRIDE form):
 * x (G,H,W,Cin), H and W even -> y (G,H/2,W/2,Cout) (+ bias, ReLU).  Built for Cout = 64, Cin % 32 == 0 (conv1_x_0/conv2 of
 * ResNetDS2SPP); weights atvs_conv2d_b_pack; stats_partial: rows atvs_conv2d_lds_rows(H/2, W/2, Cout) or NULL. */
int atvs_conv2d_b_s2_supported(int Cin, int Cout);
int atvs_conv2d_b_s2_f32(const float* x, const unsigned char* packed_w, const float* bias, float* y, double* stats_partial, int G,
                         int H, int W, int Cin, int Cout, int relu, atvs_stream_t stream);

/* 1x1 convolution of feature maps (the bottlenecks' conv1 / conv3 / shortcut, fusion1: slim.conv2d 1x1,
 * network.py:573-601; cnn_wrapper/atvsnet.py:254-292) as a tall GEMM: weights staged once per workgroup in LDS, pixels
 * streamed once (conv1x1.hip).  x (groups, pixels, Cin), Cin % 16 == 0, Cin <= 128, Cout in {32, 64, 128}.
 *   atvs_conv1x1_pack_size / _pack   HOST: pack the TF kernel [1,1,Cin,Cout]
 *   atvs_conv1x1_rows                workgroups per image = rows per image of stats_partial ([2][Cout] doubles each)
 *   atvs_conv1x1_f32                 y (groups,pixels,ldy)[..., y_coff + co] = x W (+ bias, + residual, ReLU); in_params
 *                                    (groups,3,Cin) != NULL: batch norm (+ ReLU if in_relu) of x applied on load -- the
 *                                    bottleneck's pre-activation (network.py:570-571) is never materialised. */
int atvs_conv1x1_supported(int Cin, int Cout);
int atvs_conv1x1_pack_size(int Cin, int Cout, long* packed_floats);
int atvs_conv1x1_pack(const float* w, int Cin, int Cout, float* packed);
long atvs_conv1x1_rows(long pixels);
int atvs_conv1x1_f32(const float* x, const float* packed_w, const float* bias, const float* residual,
                     const float* in_params, int in_relu, float* y, double* stats_partial, int groups, long pixels,
                     int Cin, int Cout, int ldy, int y_coff, int relu, atvs_stream_t stream);

/* The same layers (network.py:573-601) with SPLIT fp16 operands on the 16-bit matrix cores (conv1x1_b.hip; the arithmetic of
 * atvs_conv_c16b_f32): Cin % 32 == 0, Cin <= 1024, Cout in {32, 64, 128}.  Same contract as atvs_conv1x1_f32 except the
 * packed weights (bytes of fp16 pieces) and the statistics rows (128 pixels per workgroup: atvs_conv1x1_b_rows). */
int atvs_conv1x1_b_supported(int Cin, int Cout);
int atvs_conv1x1_b_pack_size(int Cin, int Cout, long* packed_bytes);
int atvs_conv1x1_b_pack(const float* w, int Cin, int Cout, unsigned char* packed);
long atvs_conv1x1_b_rows(long pixels);
int atvs_conv1x1_b_f32(const float* x, const unsigned char* packed_w, const float* bias, const float* residual,
                       const float* in_params, int in_relu, float* y, double* stats_partial, int groups, long pixels,
                       int Cin, int Cout, int ldy, int y_coff, int relu, atvs_stream_t stream);

/* One launch per pre-activation residual unit (bottleneck_b.hip; replaces Network.bottleneck, reference
 * cnn_wrapper/network.py:552-602, for depth == depth_in, stride 1 -- the identity-shortcut units of res_block, :604-616):
 *   y = x + conv3_1x1(relu(conv2_3x3_dil(relu(conv1_1x1(relu(bn(x))) + b1)) + b2)) + b3
 * for G images (H,W,C) channel-last fp32.  The unit has ONE global reduction (the moments of x, in_params (G,3,C) from
 * atvs_bn_finalize); conv1 is evaluated for the tile and its dilation halo, r1 and r2 stay in LDS as fp16 pieces.  Split fp16
 * operands, the K order and packed weights of the unfused kernels: w1 / w3 = atvs_conv1x1_b_pack of [C][C], w2 =
 * atvs_conv2d_b_pack of [3][3][C][C]; y is bit for bit what atvs_conv1x1_b_f32 -> atvs_conv2d_b_f32 -> atvs_conv1x1_b_f32 give.
 * stats_partial: NULL or (G, atvs_bottleneck_b_rows(C, H, W), 2, C) doubles: per-workgroup moments of y (the next unit's batch
 * norm).  x and y may not alias.  Shapes: atvs_bottleneck_b_supported (C in {32, 64}, dilation 1). */
int atvs_bottleneck_b_supported(int C, int dilation);
long atvs_bottleneck_b_rows(int C, int H, int W);
int atvs_bottleneck_b_f32(const float* x, const float* in_params, const unsigned char* w1, const float* b1,
                          const unsigned char* w2, const float* b2, const unsigned char* w3, const float* b3, float* y,
                          double* stats_partial, int G, int H, int W, int C, int dilation, atvs_stream_t stream);

/* 3x3x3 SAME stride-1 convolutions with Cin % 16 == 0 and 32 / 64 output channels (conv_b*_2_1, conv_b*_3_1,
 * global_refine_3dconv{2,3}_1: cnn_wrapper/atvsnet.py StackedUNet / CostVolRefineNet, network.py:172-215) with SPLIT fp16
 * operands on the 16-bit matrix cores (conv3d_b.hip; the arithmetic of atvs_conv_c16b_f32).  x (groups,D,H,W,Cin) ->
 * y (groups,D,H,W,ldy)[..., y_coff : y_coff + Cout]; stats_partial: groups * atvs_conv_c16_grid rows of [2][Cout] doubles or NULL.
 * Weights: atvs_conv3d_b_pack (HOST; size in BYTES). */
int atvs_conv3d_b_supported(int Cin, int Cout);
int atvs_conv3d_b_pack_size(int Cin, int Cout, long* packed_bytes);
int atvs_conv3d_b_pack(const float* w, int Cin, int Cout, unsigned char* packed);
int atvs_conv3d_b_f32(const float* x, const unsigned char* packed_w, const float* bias, float* y, double* stats_partial,
                      int groups, int D, int H, int W, int Cin, int Cout, int ldy, int y_coff, int relu, atvs_stream_t stream);
/* The same convolution of relu?((x - mean) * scale + beta): x a raw convolution output, in_params (groups,3,Cin) its pending
 * batch norm (conv_b*_{2,3}_1 read conv_b*_{2,3}_0, cnn_wrapper/atvsnet.py:20-26), applied per staged halo voxel -- the
 * normalised tensor is never written.  Bit for bit atvs_bn_apply followed by atvs_conv3d_b_f32. */
int atvs_conv3d_b_norm_f32(const float* x, const float* in_params, int in_relu, const unsigned char* packed_w, const float* bias,
                           float* y, double* stats_partial, int groups, int D, int H, int W, int Cin, int Cout, int ldy,
                           int y_coff, int relu, atvs_stream_t stream);

/* The STRIDE-2 form (conv_b*_2_0: 16 -> 32, conv_b*_3_0: 32 -> 64, global_refine_3dconv{2,3}_0; network.py:172-215) with split
 * fp16 operands (conv3d_s2b.hip): x (groups,D,H,W,Cin) -> y (groups,Do,Ho,Wo,ldy)[..., y_coff : y_coff + Cout], Do = ceil(D / 2) ...,
 * TF SAME padding (pad_before = (2 (Do - 1) + 3 - D) / 2 per axis).  stats_partial: groups * atvs_conv3d_s2b_grid(Do,Ho,Wo,groups)
 * rows of [2][Cout] doubles or NULL.  Weights: atvs_conv3d_s2b_pack (HOST; size in BYTES). */
int atvs_conv3d_s2b_supported(int Cin, int Cout);
long atvs_conv3d_s2b_grid(int Do, int Ho, int Wo, int groups);
int atvs_conv3d_s2b_pack_size(int Cin, int Cout, long* packed_bytes);
int atvs_conv3d_s2b_pack(const float* w, int Cin, int Cout, unsigned char* packed);
int atvs_conv3d_s2b_f32(const float* x, const unsigned char* packed_w, const float* bias, float* y, double* stats_partial,
                        int groups, int D, int H, int W, int Cin, int Cout, int ldy, int y_coff, int relu, atvs_stream_t stream);
/* ... of relu?((x - mean) * scale + beta), in_params (groups,3,Cin) the pending batch norm of the raw convolution output x (the
 * encoders conv_b*_{2,3}_0 read conv_b*_{1,2}_0, cnn_wrapper/atvsnet.py:10-12).  Bit for bit atvs_bn_apply followed by
 * atvs_conv3d_s2b_f32. */
int atvs_conv3d_s2b_norm_f32(const float* x, const float* in_params, int in_relu, const unsigned char* packed_w,
                             const float* bias, float* y, double* stats_partial, int groups, int D, int H, int W, int Cin,
                             int Cout, int ldy, int y_coff, int relu, atvs_stream_t stream);

/* atvs_deconv_up_f32's layers and contract with SPLIT operands on the 16-bit matrix cores (deconv_up_b.hip; the arithmetic of
 * atvs_conv_c16b_f32: two fp16 pieces per operand, three products, the cross terms in an accumulator of their own).  Grid /
 * statistics rows = atvs_deconv_up_b_grid (two workgroups per CU; NOT atvs_deconv_up_grid).  The packed weights of all chunks
 * stay in LDS beside two piece images where they fit; Cout 16 with more input channels re-reads one chunk's weights per stage
 * (atvs_deconv_up_b_supported).  stats_ld / stats_coff: a statistics row is [2][stats_ld] doubles and this
 * launch's channels start at column stats_coff (16, 0 = atvs_deconv_up_f32's layout): a 32-channel layer (conv_b*_4_0) runs as two
 * 16-channel launches with y_coff / stats_coff 0 and 16, ldy = stats_ld = 32.  Weights: atvs_deconv_up_b_pack (HOST; size in BYTES;
 * ATVS_ERR_ARG for a weight beyond fp16's range). */
long atvs_deconv_up_b_grid(int D, int H, int W, int Cout, int groups);
int atvs_deconv_up_b_supported(int Cin, int Cout);
int atvs_deconv_up_b_pack_size(int Cin, int Cout, long* packed_bytes);
int atvs_deconv_up_b_pack(const float* w, int Cin, int Cout, unsigned char* packed);
int atvs_deconv_up_b_f32(const float* x, const unsigned char* packed_w, float* y, double* stats_partial, int groups, int D, int H,
                         int W, int Cin, int Cout, int ldy, int y_coff, int relu, int stats_ld, int stats_coff,
                         atvs_stream_t stream);

/* atvs_deconv_up_b_f32 over the SUM of two or three volumes that is never written (the U-Net's skip adds in front of
 * conv_b*_6_0 / global_refine_3dconv6_0, reference cnn_wrapper/atvsnet.py:156-158,186-188,332-334):
 *   x_in = t(x0, params0, bit 0) + t(x1, params1, bit 1) [+ t(x2, params2, bit 2)],
 *   t(v, par, relu) = par ? relu?((v - mean) * scale + beta) : v                  (relu = that bit of relu_mask)
 * -- atvs_bn_add's arithmetic and order, formed per staged halo voxel; params_i (groups,3,Cin) or NULL (a finished tensor),
 * x2 NULL: two terms.  Bit for bit atvs_bn_add followed by atvs_deconv_up_b_f32.  Shapes: atvs_deconv_up_b_sum_supported
 * (Cin = 16, Cout = 8: the full-resolution decoder; one workgroup of eight wavefronts per CU, four multiply and store, four stage
 * the next tile's sources). */
int atvs_deconv_up_b_sum_supported(int Cin, int Cout);
int atvs_deconv_up_b_sum_f32(const float* x0, const float* params0, const float* x1, const float* params1, const float* x2,
                             const float* params2, int relu_mask, const unsigned char* packed_w, float* y, double* stats_partial,
                             int groups, int D, int H, int W, int Cin, int Cout, int ldy, int y_coff, int relu, int stats_ld,
                             int stats_coff, atvs_stream_t stream);
/* conv_bn(3, 8, 1) on a volume with ONE or TWO channels: the probability / visual-hull / geometric stems of the
 * refinement network (cnn_wrapper/atvsnet.py:300-311).  HBM-bound (432 FLOP per 36 B at one channel): FMA kernel with a
 * sliding register window along z, not MFMA (conv_stem.hip).  x (groups,D,H,W,Cin), Cin in {1,2}; w = the TF kernel
 * [3,3,3,Cin,8] on the device; y (groups,D,H,W,ldy)[..., y_coff + co]; plane_bias (groups,H,W,24) or NULL (see
 * atvs_conv_mfma_f32); stats_partial: groups * atvs_conv_stem_rows rows of [2][16] doubles (columns 0..7) or NULL. */
long atvs_conv_stem_rows(int D, int H, int W);
int atvs_conv_stem_f32(const float* x, const float* w, const float* plane_bias, float* y, double* stats_partial,
                       int groups, int D, int H, int W, int Cin, int ldy, int y_coff, int relu, atvs_stream_t stream);

/* The geo | prob | vishull stems of CostVolRefineNet (cnn_wrapper/atvsnet.py:300-313) in ONE pass, stored together with
 * the RAW output of the photo stem as whole 128-byte rows of the 32-channel concat buffer (stem-by-stem slices are
 * partial-line HBM writes): y (groups,D,H,W,32) = [photo_raw (..,8) | conv(geo (..,2)) + geo_plane_bias (groups,H,W,24) |
 * conv(prob (..,1)) | conv(hull (..,1))], no activation.  atvs_refine_stems_pack (HOST) arranges the three TF kernels
 * [3,3,3,Cin,8] as [27][geo0, geo1, prob, hull][8] (upload the 864 floats).  stats_partial: groups * atvs_conv_stem_rows
 * rows of [2][24] doubles over the 24 computed channels, or NULL.
 * y_planar != 0: y is chunk-planar instead, (groups, 4, y_planar) floats with planes of [D][H][W][8] (the layout
 * atvs_conv_xb_f32 reads with x_planar): planes 1..3 = geo | prob | hull are written, plane 0 is the photo stem's own
 * output (atvs_conv_xb_f32 with ldy = 8 and y_group_stride = 4 * y_planar) and photo_raw is not read (may be NULL):
 * 16 B read + 96 B written per voxel instead of 48 + 128. */
int atvs_refine_stems_pack(const float* w_geo, const float* w_prob, const float* w_hull, float* packed);
int atvs_refine_stems_f32(const float* photo_raw, const float* geo, const float* geo_plane_bias, const float* prob,
                          const float* hull, const float* w, float* y, double* stats_partial, int groups, int D, int H,
                          int W, long y_planar, atvs_stream_t stream);

/* conv(3, 1, 1, relu=False) on an 8-channel volume: the probability heads conv_b2_6_2,
 * attention_prob_vol[_refine], global_refined_cost_vol (cnn_wrapper/atvsnet.py:192,213,220,226,
 * 242,336).  x (D,H,W,8); w = the TF kernel [3,3,3,8,1] (216 floats, device); y (D,H,W).
 * One output channel: packed-FMA kernel with four outputs per thread, not MFMA (conv8to1.hip). */
int atvs_conv3d_8to1(const float* x, const float* w, float* y, int groups, int D, int H, int W, atvs_stream_t stream);
/* The same head over the two-term sum atvs_bn_add would form, x = relu?(bn(x0; params0)) + relu?(bn(x1; params1)) (relu_mask bit i:
 * ReLU after term i), formed while the kernel stages its halo: y is bit for bit atvs_bn_add(x0, params0, x1, params1) followed by
 * atvs_conv3d_8to1, and the sum is never written (conv_b2_6_1 -> conv_b2_6_2, global_refine_3dconv6_1 -> global_refined_cost_vol).
 * x0, x1 (groups,D,H,W,8) raw; params_i (groups,3,8).  Voxels outside the volume pad the SUM with 0.  relu_mask > 3: ATVS_ERR_ARG. */
int atvs_conv3d_8to1_bn2(const float* x0, const float* params0, const float* x1, const float* params1, int relu_mask,
                         const float* w, float* y, int groups, int D, int H, int W, atvs_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Batch norm with batch statistics, element-wise glue  (cnn_wrapper/network.py)
 * ------------------------------------------------------------------------- */

/* `groups` in this section: the tensor is `groups` INDEPENDENT samples stacked along its leading axis, each with its
 * own batch statistics -- the reference evaluates every network call with batch 1 and per-call statistics (quirk C1);
 * stacking the calls of a depth map (views, siamese directions) into one launch must not change them. */

/* Reduce per-workgroup partial sums [groups][num_blocks][2][cpad] (double) to
 * params [groups][3][C] = (mean, rsqrt(var+eps), beta): the moments of
 * tf.layers.batch_normalization(training=True) / slim.batch_norm, network.py:206-212,
 * 541-547, 570-571.  count = elements per channel of one sample.  beta (C, shared) or NULL.  fold >= 1: channel c
 * also sums columns c + C, c + 2C, ... (fold of them).  nonfinite_flag: NULL or a device word that is OR-ed with 1 when a
 * moment is not finite -- the layers upstream carried a value beyond the fp16 range of the split-operand kernels (or a
 * non-finite input); sticky, the host reads and clears it (a later ReLU can swallow the NaN, the flag keeps it). */
int atvs_bn_finalize(const double* stats_partial, int groups, long num_blocks, int cpad, int fold, long count,
                     const float* beta, float eps, float* params, int C, int* nonfinite_flag, atvs_stream_t stream);

/* Partial sums of an arbitrary (groups, rows, C) tensor, C <= 256, in the layout above with
 * cpad = C and atvs_channel_stats_num_blocks(rows) blocks per sample. */
long atvs_channel_stats_num_blocks(long rows);
int atvs_channel_stats(const float* x, int groups, long rows, int C, double* stats_partial, atvs_stream_t stream);

/* y = (x - mean) * rstd + beta [, relu]; y may alias x.  x and y are groups * rows rows of width ld of which the C
 * channels starting at c_off are touched (ld = C, c_off = 0 for a dense tensor); params (groups, 3, C).
 * Arithmetic (here and wherever an entry point of this header applies a pending batch norm while it loads -- the in_params /
 * params_i arguments): ONE fused multiply-add per value, fma(x, rstd, beta - mean * rstd), tf.nn.batch_normalization's own form
 * (x * inv + (offset - mean * inv)); every site uses the same two helpers, so a fused form equals the passes it replaces bit for bit. */
int atvs_bn_apply(const float* x, const float* params, float* y, int groups, long rows, int C, int ld, int c_off,
                  int relu, atvs_stream_t stream);

/* tf.add_n of two or three tensors of which any may still be a raw convolution output whose
 * batch norm (+ ReLU, relu_mask bit i) is pending: y = sum_i bn_relu_i(x_i), params_i (groups,3,C) or NULL
 * for an already-final tensor; x2 may be NULL.  C % 4 == 0; rows per sample.  (network.py:172-215 + :695-697 fused.) */
int atvs_bn_add(const float* x0, const float* params0, const float* x1, const float* params1, const float* x2,
                const float* params2, float* y, int groups, long rows, int C, int relu_mask, atvs_stream_t stream);
/* atvs_bn_add that also writes y2 = base + y, base (rows,C) ONE sample shared by the `groups` samples (global_refine_3dconv6_1 and
 * refined_cost = filtered_cost + cost_residual of every source view, model.py:438, in one pass): y / y2 bit for bit atvs_bn_add /
 * atvs_add_n(base, y).  y may be NULL: only y2 is written (a caller that reads no cost residual). */
int atvs_bn_add_plus(const float* x0, const float* params0, const float* x1, const float* params1, const float* x2,
                     const float* params2, float* y, const float* base, float* y2, int groups, long rows, int C, int relu_mask,
                     atvs_stream_t stream);

/* tf.add_n of two or three tensors (c may be NULL), network.py:695-697. */
int atvs_add_n(const float* a, const float* b, const float* c, float* y, long n, atvs_stream_t stream);

/* tf.layers.average_pooling2d(padding='SAME'), network.py:665-671: x (H,W,C) ->
 * y (ceil(H/stride), ceil(W/stride), C), mean over the valid window elements; `groups` images per launch.
 * ws: groups * atvs_avg_pool_ws_floats(H, W, C, stride) floats of scratch. */
long atvs_avg_pool_ws_floats(int H, int W, int C, int stride);
int atvs_avg_pool_same(const float* x, float* y, float* ws, int groups, int H, int W, int C, int pool, int stride,
                       atvs_stream_t stream);

/* tf.image.resize_images(BILINEAR, align_corners=True), network.py:649-655:
 * x (H,W,C) -> y (Ho,Wo,ld_out)[..., c_off:c_off+C]. */
int atvs_resize_bilinear(const float* x, float* y, int groups, int H, int W, int C, int Ho, int Wo, int ld_out,
                         int c_off, atvs_stream_t stream);

/* tf.concat along channels / un-stacking a trailing axis, network.py:691-693:
 * dst[r, dst_off + c] = src[r, src_off + c], c < C. */
int atvs_copy_channels(const float* src, float* dst, long rows, int C, int ld_src, int src_off, int ld_dst,
                       int dst_off, atvs_stream_t stream);

/* tf.stack along a new leading axis (model.py:186,289: the per-pair reference features of a batch of cost volumes, the two
 * initial depth maps of the refinement): dst[i] = *srcs[i], i < n <= 16, each `elems` floats (a multiple of 4, 16-byte aligned).
 * srcs: HOST array of n device pointers. */
int atvs_stack(const float* const* srcs, int n, long elems, float* dst, atvs_stream_t stream);

/* ------------------------------------------------------------------------- *
 * AANet aggregation over views  (cnn_wrapper/network.py:282-351, 378-408)
 * ------------------------------------------------------------------------- */

/* sr_ptrs / x_ptrs: HOST arrays of nv (<= 16) device pointers.  SR_n (V,16) =
 * [relu(conv(X_n, W_shared)) | relu(conv(X_n, W_unique))], X_n (V,8).
 * out (V,8) = sum_n softmax_n(R_n - S_n + sum_m S_m) * X_n. */
int atvs_aanet_combine(const float* const* sr_ptrs, const float* const* x_ptrs, int nv, float* out, long V,
                       atvs_stream_t stream);

/* The whole AANet module in ONE launch (aanet_b.hip; round 6: eight wavefronts in two roles -- four multiply, four stage the next
 * halo and run the softmax of the previous tile beside them): the shared | unique 3x3x3 score convolutions of every view (split
 * fp16 operands, conv_c16b's K order), their results handed over in LDS, then the cross-view softmax and weighted sum --
 *   out (D,H,W,8) = sum_n softmax_n((R_n - S_n) + sum_m S_m) * X_n,   S_n | R_n = relu(conv3d(X_n, W_shared | W_unique, SAME))
 * (reference cnn_wrapper/network.py:282-351,378-408).  x: HOST array of nv <= 8 device pointers (D,H,W,8) (atvs_aanet_b_supported; more views: the two-launch form); packed_w:
 * atvs_aanet_b_pack(w_shared, w_unique) (HOST; [3,3,3,8,8] each; size in BYTES).  [S|R] is never written: bit for bit
 * atvs_conv_c16b_f32 (ReLU) per view followed by atvs_aanet_combine. */
int atvs_aanet_b_supported(int C, int nv);
int atvs_aanet_b_pack_size(long* packed_bytes);
int atvs_aanet_b_pack(const float* w_shared, const float* w_unique, unsigned char* packed);
int atvs_aanet_b_f32(const float* const* x, int nv, const unsigned char* packed_w, float* out, int D, int H, int W,
                     atvs_stream_t stream);

/* The same arithmetic split at its three reductions over views, for views sharded
 * across GPUs (all-reduce SUM / MAX / SUM between stages):
 *   stage 0: out (V,8) = sum_local S_n
 *   stage 1: out (V,8) = max_local U_n                (needs ssum)
 *   stage 2: out (2,V,8) = [sum e_n ; sum e_n * X_n]   (needs ssum, umax, x_ptrs) */
int atvs_aanet_partial(const float* const* sr_ptrs, const float* const* x_ptrs, int nv, int stage,
                       const float* ssum, const float* umax, float* out, long V, atvs_stream_t stream);

/* out = num / den, n % 4 == 0 (last step of the sharded AANet). */
int atvs_divide(const float* num, const float* den, float* out, long n, atvs_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Depth-map fusion  (fusibile/fusibile.cu, after the hot path: SURVEY.md 8 f-4)
 * ------------------------------------------------------------------------- */

/* The consistency-voting kernel `fusibile` (fusibile/fusibile.cu:138-277) for reference camera `ref`.
 * cams (nviews, 28) floats per camera: P[12] (3x4 projection, row-major) | M_inv[9] (inverse of P's left 3x3) |
 * C[3] (camera centre) | P_col34[3] (P's last column) | f (K[0,0]) -- cameraGeometryUtils.h:377-433.
 * normals_depths, images: (nviews, rows, cols, 4) floats = (nx, ny, nz, depth) and (b, g, r, unused), the two float4
 * textures of main.cpp:816-822, sampled bilinearly with clamped addressing and 8-bit weights (no texture unit).
 * Outputs, all for the pixels of `ref`: coord / normal / texture (rows, cols, 4) = the pixel's 3-D point, the normal and
 * the colour averaged over the agreeing views; created (rows, cols) = 1 when at least num_consistent views agree
 * (relative disparity difference < disp_thresh and normal angle < normal_thresh), else 0. */
int atvs_fusibile(const float* cams, const float* normals_depths, const float* images, int nviews, int ref, int rows,
                  int cols, float disp_thresh, float normal_thresh, int num_consistent, float* coord, float* normal,
                  float* texture, float* created, atvs_stream_t stream);

/* One finished depth map -> its slot of a scene's fusion slab (csrc/fusion_scene.hip): per pixel what the file pipeline computes
 * on the host -- eval_pointcloud._write_map (inverse_depth = 1: a value <= 0 becomes +inf, then 1 / value, correctly rounded),
 * depth_fusion.probability_filter (depth := 0 where prob < prob_thresh) and fake_colmap_normal (each normal component
 * float32(1) / float32(1.732050808) where the depth is > 0, else +0).
 * depth, prob (rows, cols) floats; bgr (rows, cols, 3) uint8, the 1/4-scale reference image.  Outputs: nd_out (rows, cols, 4)
 * = (nx, ny, nz, depth) and img_out (rows, cols, 4) = (b, g, r, 0), the two textures atvs_fusibile / atvs_fusibile_scene read.
 * inverse_depth not 0 / 1: ATVS_ERR_ARG. */
int atvs_fusion_stage_f32(const float* depth, const float* prob, const unsigned char* bgr, int rows, int cols,
                          int inverse_depth, float prob_thresh, float* nd_out, float* img_out, atvs_stream_t stream);

/* Bytes of the scratch atvs_fusibile_scene needs for nviews maps of rows x cols (HOST call). */
int atvs_fusibile_scene_scratch_size(int nviews, int rows, int cols, long* bytes);

/* atvs_fusibile for EVERY reference camera 0 .. nviews-1 in one pass, followed by the host filter of fusibile.cu:309
 * (depth_fusion.fuse_views: keep a pixel whose point is created and has three non-zero coordinates) and a deterministic
 * compaction (three launches on `stream`: count, scan, scatter; no atomics).  Each pixel's arithmetic is atvs_fusibile's.
 * cams, normals_depths, images: as for atvs_fusibile.  scratch: atvs_fusibile_scene_scratch_size bytes (device).
 * Outputs: points (capacity, 3) floats and colors (capacity, 3) uint8 r, g, b = (uint8)(int) of texture channels 2, 1, 0, the
 * first *n_points rows written, camera-major and row-major within a camera; n_points: ONE device int.
 * capacity < nviews * rows * cols, a short scratch, or nviews * rows * cols beyond int: ATVS_ERR_SHAPE. */
int atvs_fusibile_scene(const float* cams, const float* normals_depths, const float* images, int nviews, int rows, int cols,
                        float disp_thresh, float normal_thresh, int num_consistent, void* scratch, long scratch_bytes,
                        float* points, unsigned char* colors, long capacity, int* n_points, atvs_stream_t stream);

/* atvs_fusibile_scene that also returns the normals: normals (capacity, 3) floats receives normal.xyz of atvs_fusibile for every
 * kept point, in the order of the points (the average over the reference and the agreeing views, NOT normalised).  The same
 * kernels with one more scratch region: atvs_fusibile_scene_normals_scratch_size bytes.  Points, colours and count are those of
 * atvs_fusibile_scene bit for bit. */
int atvs_fusibile_scene_normals_scratch_size(int nviews, int rows, int cols, long* bytes);
int atvs_fusibile_scene_normals(const float* cams, const float* normals_depths, const float* images, int nviews, int rows,
                                int cols, float disp_thresh, float normal_thresh, int num_consistent, void* scratch,
                                long scratch_bytes, float* points, unsigned char* colors, float* normals, long capacity,
                                int* n_points, atvs_stream_t stream);

/* The fusion's agreement count of every pixel of a scene's slab (csrc/fusion_support.hip), one launch, no images.  cams,
 * normals_depths, disp_thresh, normal_thresh as for atvs_fusibile; num_consistent >= 0.  For pixel (x, y) of camera r, `count` is
 * atvs_fusibile's count with ref = r: the number of views other than r, taken ascending, whose projection of the pixel's 3-D point
 * lies in the image, whose relative disparity difference is < disp_thresh and whose normal angle is < normal_thresh -- the same
 * float32 arithmetic, left to right, nothing contracted, the same 8-bit bilinear fetch (one function, csrc/fusion_pixel.h).
 * Three optional outputs, each (nviews, rows, cols), each may be NULL, at least one is required:
 *   count      int32: the count.
 *   depth_out  float32: the pixel's own depth normals_depths[..., 3], bit for bit, where count >= num_consistent, +0 elsewhere:
 *              the depth plane as the fusion masks its points.
 *   weight_out float32: (float)(1 + count) / (float)(1 + num_consistent), one correctly rounded float32 division, written for
 *              every pixel whatever the mask says.  A pixel that just passes the mask weighs exactly 1, a better supported one
 *              more, so the weights of the views a voxel had before never sum to less than their number.  The formula is a default,
 *              not a measurement.
 * One workgroup per (camera, run of 256 row-major pixels); no atomics, no scratch; the same inputs give the same bits.
 * All three outputs NULL: ATVS_ERR_NULL; nviews * rows * cols beyond int: ATVS_ERR_SHAPE (atvs_fusibile_scene's limits);
 * num_consistent < 0: ATVS_ERR_ARG. */
int atvs_fusion_support(const float* cams, const float* normals_depths, int nviews, int rows, int cols, float disp_thresh,
                        float normal_thresh, int num_consistent, int* count, float* depth_out, float* weight_out,
                        atvs_stream_t stream);

/* Normals of a scene's depth maps from the maps themselves (csrc/depth_normals.hip), one launch over the fusion slab
 * normals_depths (nviews, rows, cols, 4) = (nx, ny, nz, depth), IN PLACE: only .w (the depth) is read, only the three normal
 * floats are written.  cams (nviews, 28) as for atvs_fusibile.  Per pixel (x, y) with depth d, in float64:
 *   d > 0 false -> (0,0,0).  X(x,y,d) = M_inv (d x - p0, d y - p1, d - p2).  Neighbours R = (x+step, y), D = (x, y+step),
 *   L = (x-step, y), U = (x, y-step), valid when inside the image, dn > 0 and |dn - d| <= depth_gate * d.  For the quadrants
 *   (R,D), (D,L), (L,U), (U,R) with both neighbours valid: c = (Xa - X) x (Xb - X), and c / |c| is added to a sum when |c| > 0.
 *   |sum| = 0 -> (0,0,0); else n = sum / |sum|, negated when n . (C - X) < 0 (the surface faces its camera); stored as float.
 * A zero normal is 90 degrees from every normal in atvs_fusibile (acosf(0)): under a normal threshold below 90 degrees such a
 * pixel agrees with no view.
 * step < 1, depth_gate negative or not finite: ATVS_ERR_ARG; nviews * rows * cols beyond int: ATVS_ERR_SHAPE. */
int atvs_depth_normals_f32(const float* cams, float* normals_depths, int nviews, int rows, int cols, int step, float depth_gate,
                           atvs_stream_t stream);


/* ---- 3x3x3 stride-2 SAME transposed convolution to 8 or 16 channels, all 8 output parity classes per staged input tile
 * (csrc/deconv_up.hip): the decoders conv_b*_6_0 / conv_b*_5_0, global_refine_3dconv6_0 / 5_0 (cnn_wrapper/atvsnet.py
 * StackedUNet / CostVolRefineNet; tf.layers.conv3d_transpose, cnn_wrapper/network.py:510-550).  Cout in {8, 16},
 * Cin % 16 == 0, Cin <= 64, output below 4 GiB per sample (else ATVS_ERR_SHAPE: callers use the class-fused form of
 * atvs_conv_tiled_f32).
 * w: TF layout [3,3,3,Cout,Cin].  x (groups, D,H,W, Cin) -> y (groups, 2D,2H,2W, ldy)[..., y_coff : y_coff + Cout].
 * stats_partial: groups * atvs_deconv_up_grid rows of [2][16] doubles (sum / sum of squares per channel) or NULL. */
int atvs_deconv_up_pack_size(int Cin, int Cout, long* packed_floats);
int atvs_deconv_up_pack(const float* w, int Cin, int Cout, float* packed);        /* host function */
long atvs_deconv_up_grid(int D, int H, int W, int Cout, int groups);              /* workgroups PER SAMPLE */
int atvs_deconv_up_f32(const float* x, const float* packed_w, float* y, double* stats_partial, int groups, int D, int H,
                       int W, int Cin, int Cout, int ldy, int y_coff, int relu, atvs_stream_t stream);

/* ---- 3x3x3 SAME stride-1 convolution to 16 channels (Cin in {8, 16, 32}) or 32 channels (Cin in {16, 32, 48, 64}), one
 * workgroup per CU (csrc/conv_c16.hip): the half- / quarter-resolution layers conv_b*_1_1, conv_b*_2_1,
 * global_refine_3dconv1_1 / 2_1 (cnn_wrapper/atvsnet.py StackedUNet / CostVolRefineNet; cnn_wrapper/network.py:165-215)
 * and the AANet modules' shared | unique convolution (network.py:282-351, 8 -> 8 + 8).  Other shapes: ATVS_ERR_SHAPE
 * (callers use atvs_conv_tiled_f32).
 * w: TF layout [3,3,3,Cin,Cout].  x (groups, D,H,W, Cin) -> y (groups, D,H,W, ldy)[..., y_coff : y_coff + Cout] (+ bias,
 * ReLU).  stats_partial: groups * atvs_conv_c16_grid rows of [2][Cout] doubles (sum / sum of squares per channel) or NULL. */
int atvs_conv_c16_pack_size(int Cin, int Cout, long* packed_floats);
int atvs_conv_c16_pack(const float* w, int Cin, int Cout, float* packed);         /* host function */
long atvs_conv_c16_grid(int D, int H, int W, int groups);                         /* workgroups PER SAMPLE */
int atvs_conv_c16_f32(const float* x, const float* packed_w, const float* bias, float* y, double* stats_partial,
                      int groups, int D, int H, int W, int Cin, int Cout, int ldy, int y_coff, int relu,
                      atvs_stream_t stream);

/* The 8 / 16 -> 16 channel forms of atvs_conv_c16_f32 on the 16-bit matrix cores with SPLIT operands (conv_c16b.hip;
 * BASELINE.json configs[1] names "bf16 conv3d MFMA"): x = h0 + h1 / 2048 and w = g0 + g1 / 2048 in fp16 (h0 = fp16(x),
 * h1 = fp16((x - h0) * 2048): 22 significant bits, the residual piece scaled into fp16's normal range), the three products
 * h0 g0 + (h0 g1 + h1 g0) / 2048 accumulated in fp32 by v_mfma_f32_16x16x32_f16, the cross terms in an accumulator of their
 * own that is scaled once -- fp32-class results (per-layer error against float64 below the fp32 MFMA form's; rounding
 * differs from it).  |x| or |w| beyond 65504 gives inf / NaN; the packers return ATVS_ERR_ARG for such weights.  Same grid /
 * statistics rows as atvs_conv_c16_f32.
 *   atvs_conv_c16b_pack_size / _pack   HOST: split and pack the TF kernel [3,3,3,Cin,16], Cin 8 or 16 (bytes; upload the result) */
int atvs_conv_c16b_pack_size(int Cin, long* packed_bytes);
int atvs_conv_c16b_pack(const float* w, int Cin, unsigned char* packed);
int atvs_conv_c16b_f32(const float* x, const unsigned char* packed_w, const float* bias, float* y, double* stats_partial,
                       int groups, int D, int H, int W, int Cin, int ldy, int y_coff, int relu, atvs_stream_t stream);
/* The 16 -> 16 form of an input that is never written: x_in = t(x0, params0, bit 0) [+ t(x1, params1, bit 1)] with
 * t(v, par, relu) = par ? relu?((v - mean) * scale + beta) : v -- one term: a pending batch norm applied while the halo is staged
 * (conv_b0_1_1 reads conv_b0_1_0; atvs_bn_apply's arithmetic); two terms: the U-Net's skip sum (conv_b{1,2}_1_1_concat,
 * cnn_wrapper/atvsnet.py:45-46,75-76,140-141,170-171; atvs_bn_add's arithmetic and order).  params_i (groups,3,16) or NULL (that
 * term is a finished tensor); x1 NULL: one term (params0 required).  relu_mask bit i: ReLU after term i's batch norm.  Bit for
 * bit atvs_bn_apply / atvs_bn_add followed by atvs_conv_c16b_f32. */
int atvs_conv_c16b_sum_supported(int Cin);
int atvs_conv_c16b_sum_f32(const float* x0, const float* params0, const float* x1, const float* params1, int relu_mask,
                           const unsigned char* packed_w, const float* bias, float* y, double* stats_partial, int groups, int D,
                           int H, int W, int Cin, int ldy, int y_coff, int relu, atvs_stream_t stream);

/* View preparation of the scene driver (eval_pointcloud --scene_cache), csrc/prepare.hip.  Images are uint8 BGR (h,w,3).
 * atvs_prepare_resize_u8: cv2.resize(INTER_LINEAR) of 8-bit images exactly as preprocess.scale_image computes it, for the
 * output rows / columns the host lists: ytap (4,H) and xtap (4,W) int32 = (left index, right index, left weight, right weight),
 * the 11-bit weights preprocess.py forms (a centre crop is a slice of the full lists).  src (h,w,3) -> dst (H,W,3).  sums: NULL,
 * or 6 unsigned 64-bit words set to (sum x, sum x^2) of each channel of dst (zeroed on the stream, then integer atomics).
 * atvs_prepare_center: y (pixels,3) float32 = (x - mu) / (sd + 1e-8f) per channel (center_image), mu and sd from those sums in
 * double, each rounded once to float32.  pixels <= 11e6. */
int atvs_prepare_resize_u8(const unsigned char* src, int h, int w, unsigned char* dst, int H, int W, const int* ytap,
                           const int* xtap, unsigned long long* sums, atvs_stream_t stream);
int atvs_prepare_center(const unsigned char* x, long pixels, const unsigned long long* sums, float* y, atvs_stream_t stream);

/* COLMAP model import (atvsnet/colmap.py, csrc/colmap.hip).  Pointers are device pointers to the types named.
 *
 * atvs_colmap_depth_range: ColmapSparse.estimate_max_disparities (atvsnet/colmap_helpers.py:317-331) without its sort.  points
 * (n_points, 3) doubles X, Y, Z; cams (n_images, 18) doubles per image = R (3x3, row-major, world to camera), t (3), fx, fy, cx,
 * cy, width, height.  For every (image, point) pair, in float64: c_k = ((R_k0 X + R_k1 Y) + R_k2 Z) + t_k, x = (c_0 / c_2) fx + cx,
 * y = (c_1 / c_2) fy + cy, d = 1 / c_2; the point is in view when x >= 0, x < width, y >= 0, y < height and d > 0 (:322-327).
 * Outputs per image: n_in_view (int), d_lo = the in-view disparities' order statistic of rank int(n * (1 - percentile)) and d_hi
 * that of rank int(n * percentile) (:328-331 before the stretch; ranks formed in double as Python forms them), both exact (a radix
 * select on the bit patterns, integer atomics only: deterministic); 0.0 where n is 0.  scratch:
 * atvs_colmap_depth_range_scratch_size bytes (device; O(n_images), no images x points buffer).  Sixteen launches on `stream`.
 * percentile outside (0, 1): ATVS_ERR_ARG; n_images outside [1, 524280], n_points beyond int or a short scratch: ATVS_ERR_SHAPE. */
int atvs_colmap_depth_range_scratch_size(int n_images, long* bytes);
int atvs_colmap_depth_range(const double* points, long n_points, const double* cams, int n_images, double percentile, void* scratch,
                            long scratch_bytes, int* n_in_view, double* d_lo, double* d_hi, atvs_stream_t stream);

/* atvs_colmap_covisibility: the shared-point counts of ColmapSparse.generate_neighbor_list (colmap_helpers.py:333-347,
 * len(set_i & set_j)).  Tracks in CSR form: offsets (n_tracks + 1) int32, observers (n_obs) int32 image indices; each track lists
 * the DISTINCT images observing one 3-D point.  covis (n_images, n_images) int32 is zeroed, then every ordered pair (i, j), i != j,
 * of every track adds one to covis[i][j] (integer atomics; a track's pairs spread over a wave's lanes).  Tracks with an index
 * outside the arrays add nothing.  n_images above 16384 (a matrix beyond 1 GiB) or below 1: ATVS_ERR_SHAPE. */
int atvs_colmap_covisibility(const int* offsets, const int* observers, int n_tracks, int n_obs, int n_images, int* covis,
                             atvs_stream_t stream);

/* Undistortion of COLMAP's distorted camera models (atvsnet/undistort.py, csrc/undistort.hip): what
 * `colmap image_undistorter` does to the images, restated.  model_id is COLMAP's camera model id: 2 SIMPLE_RADIAL (f, cx, cy, k),
 * 3 RADIAL (f, cx, cy, k1, k2), 4 OPENCV (fx, fy, cx, cy, k1, k2, p1, p2), 5 OPENCV_FISHEYE (fx, fy, cx, cy, k1, k2, k3, k4),
 * 6 FULL_OPENCV (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6), 8 SIMPLE_RADIAL_FISHEYE (f, cx, cy, k), 9 RADIAL_FISHEYE
 * (f, cx, cy, k1, k2), 10 THIN_PRISM_FISHEYE (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, sx1, sy1).  params: HOST, 12 doubles, the
 * model's parameters in COLMAP's order, the rest ignored.  W x H: the distorted camera's size.
 *
 * atvs_undistort_map: one map per CAMERA.  camera: HOST, 4 doubles fx, fy, cx', cy' of the undistorted pinhole camera of
 * Wo x Ho pixels.  map (Ho, Wo, 2) int32, device.  One thread per output pixel (X, Y), in float64, every operation rounded,
 * nothing contracted: u = ((X + 0.5) - cx') / fx, v = ((Y + 0.5) - cy') / fy; (u_d, v_d) = the model's forward distortion in the
 * operation order of DESIGN.md 11.1 (r4 = r2 r2, r6 = r4 r2, r8 = r6 r2; the fisheye models go through atan); the source
 * coordinate s = ((fxs u_d + cxs) - 0.5, (fys v_d + cys) - 0.5) with the DISTORTED camera's fxs, fys, cxs, cys; stored in 22.10
 * fixed point, q = floor(s 1024 + 0.5).  A pixel is valid iff both s are finite and 0 <= q_x <= (W - 1) 1024, 0 <= q_y <=
 * (H - 1) 1024, decided in float64 before the conversion; an invalid pixel stores (INT32_MIN, 0).
 *
 * atvs_undistort_remap: a gather.  src (H, W, 3) uint8, map (Ho, Wo, 2) int32 (16-byte aligned), dst (Ho, Wo, 3) uint8 (4-byte
 * aligned), device.  Per output pixel: q_x = INT32_MIN gives 0 0 0; else i = q >> 10, f = q & 1023 per axis, taps at i and
 * min(i + 1, size - 1) (both clamped into the source, so no map makes the kernel read outside src), and per channel, in integers,
 * top = p00 (1024 - f_x) + p01 f_x, bot likewise from the lower row, out = (top (1024 - f_y) + bot f_y + 2^19) >> 20.  Four
 * consecutive pixels of the flat (Ho Wo) order per thread: three dword stores; the last thread finishes Ho Wo mod 4 pixels by bytes.
 *
 * Both: an unknown model_id, a non-finite parameter or camera value, fx or fy of 0, a size < 1, W or H above 2^21, W H or Wo Ho
 * beyond the int32 pixel index, a misaligned map or dst: ATVS_ERR_ARG. */
int atvs_undistort_map(int model_id, const double* params, int W, int H, const double* camera, int Wo, int Ho, int* map,
                       atvs_stream_t stream);
int atvs_undistort_remap(const unsigned char* src, int W, int H, const int* map, int Wo, int Ho, unsigned char* dst,
                         atvs_stream_t stream);

/* Point-cloud scoring (ops/cloud.py, atvsnet/eval_cloud.py, csrc/cloud.hip).  Pointers are device pointers unless named host.
 *
 * The definition.  Reference cloud P (n,3) float32, query cloud Q (m,3) float32, radius R > 0 (float32).  For a finite query q
 * and a finite reference point p: dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z and d2 = (dx*dx + dy*dy) + dz*dz, every
 * operation rounded to float32, nothing contracted.  Per query: d2min = the minimum of d2 over all finite reference points and
 * idx = the LOWEST reference index that attains it; if (double)d2min > (double)R * (double)R, or the query is not finite, or no
 * reference point is finite: d2min = +inf, idx = -1.  Non-finite reference points are never neighbours.  The result depends on
 * P, Q and R only (not on the grid's cell size or origin, the order of points inside a cell, or the launch shape): integer
 * atomics and a 64-bit integer minimum of (bits(d2) << 32) | index, no float atomics.
 *
 * atvs_cloud_grid_build: a uniform grid over the finite points of `points` (n,3), built by counting sort (bounding box by a
 * reduction kernel, per-cell counts, exclusive scan, scatter into 16-byte records x, y, z, index).  The cell edge is at least
 * R (1 + 2^-20) -- csrc/cloud.hip says why a 27-cell search is then exact -- and larger where the box would need more than
 * max(4096, min(8 n, 2^28)) cells.  `grid`: atvs_cloud_grid_scratch_size(n) bytes, O(n + cells), owned by the caller; it IS the
 * grid afterwards, valid for any number of atvs_cloud_nearest calls with the same n.  No host synchronisation.
 * atvs_cloud_nearest: queries (m,3) -> d2 (m) float32, idx (m) int32 as defined above; the queries are sorted by cell and
 * answered in that order, the results written to their original positions.  scratch: atvs_cloud_nearest_scratch_size(n, m) bytes.
 * atvs_cloud_counts: counts (ATVS_CLOUD_MAX_TOLERANCES int64, zeroed on the stream) [t] = the number of i with
 * (double)d2[i] <= tolerances[t]^2 (the square formed in double), t < k <= ATVS_CLOUD_MAX_TOLERANCES; `tolerances` is a HOST array
 * of k doubles; radius = the R d2 was computed with.
 * R <= 0 or not finite, a tolerance negative, NaN or above R: ATVS_ERR_ARG; n or m negative or beyond 2^30, a short grid or
 * scratch, k outside [1, ATVS_CLOUD_MAX_TOLERANCES]: ATVS_ERR_SHAPE.  n = 0 and m = 0 are valid (every query not found; nothing
 * launched over no points). */
#define ATVS_CLOUD_MAX_TOLERANCES 16
int atvs_cloud_grid_scratch_size(long n, long* bytes);
int atvs_cloud_grid_build(const float* points, long n, float radius, void* grid, long grid_bytes, atvs_stream_t stream);
int atvs_cloud_nearest_scratch_size(long n, long m, long* bytes);
int atvs_cloud_nearest(const void* grid, long grid_bytes, long n, const float* queries, long m, void* scratch, long scratch_bytes,
                       float* d2, int* idx, atvs_stream_t stream);
int atvs_cloud_counts(const float* d2, long m, const double* tolerances, int k, float radius, long long* counts,
                      atvs_stream_t stream);

/* Point-cloud registration (ops/cloud.py, atvsnet/register_cloud.py, csrc/cloud_register.hip).  Pointers are device pointers unless
 * named host.  Integer atomics only: every output is a function of the inputs alone, bit for bit on every run.  No host
 * synchronisation; scratch is the caller's.  tests/cloud_register_restated.py restates the first three definitions,
 * tests/cloud_plane_restated.py the plane moments.
 *
 * atvs_cloud_transform: out (n,3) float32 = points (n,3) through matrix12 (HOST, 12 doubles: rows 0-2 of a 4x4 matrix, row-major;
 * copied into the launch).  Per point and output coordinate k, in double: ((T[k][0] x + T[k][1] y) + T[k][2] z) + T[k][3], every
 * operation rounded to double, the result rounded once to float32.  Non-finite inputs propagate as IEEE gives them.  `out` may be
 * `points`.
 *
 * atvs_cloud_pair_moments: src (m,3) float32 = the queries as they were searched, dst (n,3) float32 = the searched cloud in its
 * original order, idx (m) int32 and d2 (m) float32 = what atvs_cloud_nearest returned.  Pair i takes part when 0 <= idx[i] < n and
 * (double)d2[i] <= trim * trim (trim a double >= 0, +inf allowed; a NaN d2 takes no part).  With a = (double)src[i] - pivot_src and
 * b = (double)dst[idx[i]] - pivot_dst (pivots: HOST, 3 finite doubles each, chosen by the caller so that the sums do not cancel far
 * from the origin), `out` receives 19 8-byte words: [0] the pair count (int64), then 18 doubles: [1..3] sum a, [4..6] sum b,
 * [7..15] sum a_r * b_c (row r of a: [7 + 3 r + c]), [16] sum (a0 a0 + a1 a1) + a2 a2, [17] sum (b0 b0 + b1 b1) + b2 b2,
 * [18] sum (double)d2.  Every term is formed in double as written, each product and sum rounded.  The reduction has a FIXED shape
 * (csrc/cloud_register.hip): an accumulator sees at most L = ATVS_CLOUD_MOMENT_RUN serial additions, then per-workgroup partial
 * rows are folded by fixed trees in index order, at most L + ceil(log2 m) rounding additions deep in all.  m = 0: 19 zero words.
 * scratch: atvs_cloud_pair_moments_scratch_size(m) bytes.  trim negative or NaN, a non-finite pivot: ATVS_ERR_ARG.
 *
 * atvs_cloud_plane_moments: the sums of one Gauss-Newton step of point-to-plane ICP over the SOURCE's normals.  src (m,3) float32 =
 * the original, unmoved source; normals (m,3) float32 = its normals in its own frame; matrix12 (HOST, 12 doubles) = the current T
 * as atvs_cloud_transform takes it; rot9 (HOST, 9 doubles, row-major) = the pure rotation of T (the caller divides a scale out);
 * dst (n,3), idx (m), d2 (m) = the searched cloud and what atvs_cloud_nearest returned for atvs_cloud_transform(src, T); pivot
 * (HOST, 3 finite doubles) in dst's frame.  Pair i takes part under atvs_cloud_pair_moments' rule (0 <= idx[i] < n, (double)d2[i]
 * <= trim * trim, a NaN d2 takes no part) when in addition its three normal components are finite and (nx nx + ny ny) + nz nz > 0
 * in double (a zero normal agrees with nothing).  Per pair, in double, every operation rounded on its own:
 *   q_k  = (((T[k][0] x + T[k][1] y) + T[k][2] z) + T[k][3]) - pivot_k      (atvs_cloud_transform's order, NOT rounded to float32)
 *   g_k  = (double)dst[idx[i]]_k - pivot_k
 *   n'_k = (rot[k][0] nx + rot[k][1] ny) + rot[k][2] nz                       (not renormalised: a pair weighs by |n|^2)
 *   r    = ((q_0 - g_0) n'_0 + (q_1 - g_1) n'_1) + (q_2 - g_2) n'_2
 *   J    = [ g_1 n'_2 - g_2 n'_1,  g_2 n'_0 - g_0 n'_2,  g_0 n'_1 - g_1 n'_0,  n'_0,  n'_1,  n'_2,  (q_0 n'_0 + q_1 n'_1) + q_2 n'_2 ]
 * J is the gradient of r under a small motion about the pivot, x -> pivot + (1 + sigma) Exp(omega) (x - pivot) + t, applied to the
 * moved source AND to its normals (n' -> Exp(omega) n'), in the unknowns (omega, t, sigma).  To first order, with Exp(omega) v =
 * v + omega x v:  r' = (q + omega x q + sigma q + t - g) . (n' + omega x n')
 *                    = r + omega . (q x n') + omega . (n' x (q - g)) + t . n' + sigma q . n'
 *                    = r + omega . (g x n') + t . n' + sigma q . n'
 * (the q x n' of the moving point cancels against the turning normal: what is left is the TARGET's lever arm g x n').  `out`
 * receives 38 8-byte words: [0] the pair count (int64), then 37 doubles: [1..28] sum J_a J_b for a <= b, row-major over the upper
 * triangle ([1 + 7 a - a (a - 1) / 2 + (b - a)]), [29..35] sum J_a r, [36] sum r r, [37] sum (double)d2.  The normal equations of
 * the step are (sum J J^T) (omega, t, sigma) = -sum J r; a rigid step takes their first six rows and columns.  The reduction is
 * atvs_cloud_pair_moments' (no atomics; at most L + ceil(log2 m) rounding additions deep; the same input gives the same 38 words
 * bit for bit).  m = 0: 38 zero words.  scratch: atvs_cloud_plane_moments_scratch_size(m) bytes.  trim negative or NaN, a
 * non-finite pivot, matrix12 or rot9 entry: ATVS_ERR_ARG.
 *
 * atvs_cloud_plane_moments_target: the same step over the TARGET's normals (Chen and Medioni's form).  dst_normals (n,3) float32 =
 * one normal per row of dst, in dst's frame; the pair's normal is n = (double)dst_normals[idx[i]], used as it is: nothing is rotated,
 * there is no rot9.  Pair i takes part under atvs_cloud_plane_moments' rule with that normal in the place of the source's (finite,
 * (n_0 n_0 + n_1 n_1) + n_2 n_2 > 0 in double).  q_k and g_k are as above (q NOT rounded to float32), and
 *   r    = ((q_0 - g_0) n_0 + (q_1 - g_1) n_1) + (q_2 - g_2) n_2
 *   J    = [ q_1 n_2 - q_2 n_1,  q_2 n_0 - q_0 n_2,  q_0 n_1 - q_1 n_0,  n_0,  n_1,  n_2,  (q_0 n_0 + q_1 n_1) + q_2 n_2 ]
 * The normal does not move with the source, so to first order r' = (q + omega x q + sigma q + t - g) . n =
 * r + omega . (q x n) + t . n + sigma q . n: the lever arm is the moved SOURCE's, q x n.  r and every J_a change sign with n (negation is
 * exact), so every product J_a J_b, J_a r and r r keeps its bits: negating any normals changes no bit of `out`.  The 38 words, their
 * layout, the reduction, m = 0, the scratch size (atvs_cloud_plane_moments_target_scratch_size(m) = the source form's) and the error
 * codes are atvs_cloud_plane_moments'.
 *
 * atvs_cloud_voxel_downsample: one output point per occupied cubic voxel of edge `voxel` (double > 0): the mean of the voxel's
 * finite points; non-finite points are dropped.  origin: HOST, 3 finite doubles.  Per axis, in double: g = ((double)x - origin) /
 * voxel, c = floor(g), u = (uint64)floor((g - c) * 2^32) clamped to 2^32 - 1.  A voxel is the triple of c, packed 3 x 21 bits as
 * the key of an open-addressing hash table (capacity = the power of two >= max(2 n, 1024); 64-bit compare-and-swap); its slot
 * holds the count k, the three exact unsigned 64-bit sums S of u and the lowest original index.  The output coordinate is
 * origin + voxel * ((double)c + ((double)S / (double)k) / 2^32), rounded once to float32.  Output order: ascending lowest original
 * index of the voxel; out_first (k) int32 is that index, out_points (k,3) the means (both with room for n rows), out_count (one
 * int64, device) the number of voxels.  A finite point whose cell coordinate leaves [0, 2^21) on an axis makes the call a
 * shape error that only the device can see: out_count is -1 and out_points / out_first are not written (ops/cloud.py raises).
 * scratch: atvs_cloud_voxel_downsample_scratch_size(n) bytes (40 B per slot, 8 B per point).  voxel <= 0 or not finite, a
 * non-finite origin: ATVS_ERR_ARG.  n or m negative or beyond 2^30, a short scratch: ATVS_ERR_SHAPE. */
#define ATVS_CLOUD_MOMENT_RUN 16
int atvs_cloud_transform(const float* points, long n, const double* matrix12, float* out, atvs_stream_t stream);
int atvs_cloud_pair_moments_scratch_size(long m, long* bytes);
int atvs_cloud_pair_moments(const float* src, const float* dst, long n, const int* idx, const float* d2, long m, double trim,
                            const double* pivot_src, const double* pivot_dst, void* scratch, long scratch_bytes, void* out,
                            atvs_stream_t stream);
int atvs_cloud_plane_moments_scratch_size(long m, long* bytes);
int atvs_cloud_plane_moments(const float* src, const float* normals, const double* matrix12, const double* rot9, const float* dst,
                             long n, const int* idx, const float* d2, long m, double trim, const double* pivot, void* scratch,
                             long scratch_bytes, void* out, atvs_stream_t stream);
int atvs_cloud_plane_moments_target_scratch_size(long m, long* bytes);
int atvs_cloud_plane_moments_target(const float* src, const double* matrix12, const float* dst, const float* dst_normals, long n,
                                    const int* idx, const float* d2, long m, double trim, const double* pivot, void* scratch,
                                    long scratch_bytes, void* out, atvs_stream_t stream);
int atvs_cloud_voxel_downsample_scratch_size(long n, long* bytes);
int atvs_cloud_voxel_downsample(const float* points, long n, double voxel, const double* origin, void* scratch, long scratch_bytes,
                                float* out_points, long long* out_count, int* out_first, atvs_stream_t stream);

/* Point-cloud neighbourhoods (ops/cloud.py, atvsnet/clean_cloud.py, csrc/cloud_knn.hip): the k nearest reference points, the
 * number of reference points inside the radius, and the statistics of statistical outlier removal.  Pointers are device pointers.
 * No float atomics, no host synchronisation, no allocation; scratch is the caller's.  tests/cloud_knn_restated.py restates the
 * definitions.  `grid` is a grid of atvs_cloud_grid_build over a reference cloud P (n,3) with radius R; Q (m,3) are the queries.
 *
 * Candidates.  A candidate of query j is every finite reference point i, except i == j when exclude_same_index is set (a cloud
 * searched in itself: m must equal n; ONE index is excluded, not a position: a duplicate of the query at another index is a
 * neighbour at distance 0).  d2 is the float32 expression above, (dx*dx + dy*dy) + dz*dz.  A candidate is kept when
 * (double)d2 <= (double)R * (double)R.  Kept candidates are ordered by (bits(d2), i) ascending -- the 64-bit key
 * (bits(d2) << 32) | i that atvs_cloud_nearest minimises.  A non-finite query, or one further than a cell outside the grid, has no
 * candidate.
 *
 * atvs_cloud_knn: d2 (m,k) float32 and idx (m,k) int32, 1 <= k <= ATVS_CLOUD_MAX_K: per query the first k keys of that order,
 * padded with (+inf, -1).  With k = 1 and the flag clear it is atvs_cloud_nearest bit for bit.  The output depends on P, Q, R, k
 * and the flag only.  scratch: atvs_cloud_knn_scratch_size(n, m) bytes (the queries' counting sort, as for atvs_cloud_nearest).
 * atvs_cloud_radius_count: count (m) int32 = the number of kept candidates; the same scratch.
 * atvs_cloud_knn_mean: d2 (m,k) of atvs_cloud_knn -> s (m) float64: where all k entries are finite
 * s = (sum_t sqrt((double)d2[j,t])) / k, added in ascending t from +0, every operation rounded to double; otherwise +inf (the k-th
 * neighbour lies beyond the radius).
 * atvs_cloud_sor_stats: s (m) float64 -> out, three 8-byte words: [0] c = the number of finite entries (int64), [1] their mean
 * mu = (sum s) / c (double; 0 when c = 0), [2] sigma = sqrt((sum (s - mu)^2) / (c - 1)) (double; 0 when c < 2): the sample form
 * PCL and Open3D use.  Two passes over s; the second reads mu from the first one's result on the device.  Both sums have the fixed
 * shape of atvs_cloud_pair_moments (ATVS_CLOUD_MOMENT_RUN serial additions, then fixed trees in index order): no atomics, the
 * same s gives the same three words bit for bit.  scratch: atvs_cloud_sor_stats_scratch_size(m) bytes.  m = 0: three zero words.
 * atvs_cloud_bounds: out, eight 4-byte words: [0..2] the minimum, [3..5] the maximum x, y, z (float32) over the finite rows of
 * points (n,3), [6] 1 when there is a finite row, else 0 (and [0..5] are 0), [7] 0.  The bounding-box pass of
 * atvs_cloud_grid_build (integer atomic max on order-preserving bit patterns).
 * k outside [1, ATVS_CLOUD_MAX_K], n or m negative or beyond 2^30, exclude_same_index with m != n, a short grid or scratch:
 * ATVS_ERR_SHAPE.  m = 0 is valid (nothing is written). */
#define ATVS_CLOUD_MAX_K 32
int atvs_cloud_knn_scratch_size(long n, long m, long* bytes);
int atvs_cloud_knn(const void* grid, long grid_bytes, long n, const float* queries, long m, int k, int exclude_same_index,
                   void* scratch, long scratch_bytes, float* d2, int* idx, atvs_stream_t stream);
int atvs_cloud_radius_count(const void* grid, long grid_bytes, long n, const float* queries, long m, int exclude_same_index,
                            void* scratch, long scratch_bytes, int* count, atvs_stream_t stream);
int atvs_cloud_knn_mean(const float* d2, long m, int k, double* s, atvs_stream_t stream);
int atvs_cloud_sor_stats_scratch_size(long m, long* bytes);
int atvs_cloud_sor_stats(const double* s, long m, void* scratch, long scratch_bytes, void* out, atvs_stream_t stream);
int atvs_cloud_bounds(const float* points, long n, void* out, atvs_stream_t stream);

/* Normals of an arbitrary cloud (ops/cloud.py cloud_normals, atvsnet/register_cloud.py, atvsnet/cloud_normals.py,
 * csrc/cloud_normals.hip): per query the direction of least variance of the neighbours atvs_cloud_knn found.  Pointers are device
 * pointers.  No atomics, no host synchronisation, no allocation, one launch; a row's output is a function of that row's inputs alone,
 * bit for bit on every run.  tests/cloud_normals_restated.py restates the definition.
 *
 * atvs_cloud_normals.  points P (n,3) float32 = the searched cloud, queries Q (m,3) float32, idx (m,k) int32 as atvs_cloud_knn
 * returns it for Q in P (1 <= k <= ATVS_CLOUD_MAX_K; a negative entry is padding), self_counts 0 or 1, viewpoints (v,3) DOUBLES (or
 * NULL with v = 0), view_of (m) int32 or NULL -> normals (m,3) float32 and, unless NULL, variation (m) float32.
 * Per row j, in double, every operation rounded on its own, nothing contracted:
 *   the samples   d_t = (double)P[idx[j,t]] - (double)Q[j] per component, for the t with idx[j,t] >= 0, in ascending t.  A
 *                 difference of two float32 is exact in double when their exponents differ by at most 29 (53 - 24): for every finite
 *                 pair whose larger magnitude is below 2^29 times the smaller one's last place -- any cloud whose extent is below
 *                 2^29 times its float32 spacing, which a float32 cloud with a radius search always is; beyond that it is rounded once.
 *   the sums      s = sum d_t (3) and S_ab = sum d_ta d_tb (6, a <= b), each from +0 in ascending t, product then addition.
 *   the count     c = the number of samples, + 1 when self_counts (the query is itself a sample, d = 0: the self-search with
 *                 exclude_same_index; PCL and Open3D count the point too).
 *   the matrix    C_ab = S_ab - (s_a s_b) / c.  Shifting by the query keeps every term at the neighbourhood's own scale, so this
 *                 one-pass form does not cancel however far the cloud lies from the origin: |d| is at most the search radius, so S_ab and
 *                 s_a s_b / c are at most c radius^2, the size of C's own entries, not of the squared coordinates.
 *   the normal    the unit eigenvector of the smallest eigenvalue of C, by cyclic Jacobi of FIXED shape: 6 sweeps of the rotations
 *                 (p,q) = (0,1), (0,2), (1,2), all 18 always.  A rotation, r the third index: theta = (a_qq - a_pp) / (2 a_pq);
 *                 t = sign(theta) / (|theta| + sqrt(theta theta + 1)), t = 0 when a_pq == 0; c = 1 / sqrt(t t + 1); s = t c;
 *                 a_pp = a_pp - t a_pq; a_qq = a_qq + t a_pq; a_pq = 0; (a_pr, a_qr) = (c a_pr - s a_qr, s a_pr + c a_qr);
 *                 columns p, q of V (the identity at first) turn the same way.  Afterwards lambda = the diagonal, the normal = the
 *                 column of V under the smallest entry (the lowest index on ties), lambda_0 <= lambda_1 <= lambda_2 its order.
 *                 At most 7 roundings reach an entry per rotation: the solver's backward error is at most S = 128 (>= 18 x 7) units
 *                 of 2^-53 |C|, an allowance from the operation count.  The column is unit to that error and is not renormalised.
 *   zero normal   (0, 0, 0), and variation NaN, when c < 3; when the query or a sample is not finite; when an idx[j,t] >= n (never
 *                 read); when lambda_1 <= 1e-12 lambda_2 (fewer than two directions: collinear or coincident samples) or an
 *                 eigenvalue is not finite.  This is the normal atvs_cloud_plane_moments(_target) skip.
 *   the sign      with v = view_of ? view_of[j] : 0 and 0 <= v < the number of viewpoints: e = viewpoints[v] - (double)Q[j],
 *                 dot = (n_0 e_0 + n_1 e_1) + n_2 e_2; negated when dot < 0, kept when dot > 0.  Otherwise (no viewpoints, v outside
 *                 the range -- -1 means "do not orient" --, dot == 0 or NaN): the canonical sign, the component of largest
 *                 magnitude (lowest index on ties) is made positive.  No propagation across the cloud.
 *   the outputs   normals = the three doubles rounded once to float32; variation = (float)(lambda_0 / ((lambda_0 + lambda_1) +
 *                 lambda_2)), the surface variation of Pauly et al. (it can be a rounding below 0 on an exact plane).
 * One lane per query; a lane reads its own row of idx and gathers k x 12 bytes.  m = 0 is valid (nothing is written).
 * n or m negative or beyond 2^30, k outside [1, ATVS_CLOUD_MAX_K], a negative number of viewpoints: ATVS_ERR_SHAPE; self_counts not
 * 0 or 1, viewpoints NULL with a count or a count of 0 with viewpoints, view_of without viewpoints: ATVS_ERR_ARG. */
int atvs_cloud_normals(const float* points, long n, const float* queries, long m, const int* idx, int k, int self_counts,
                       const double* viewpoints, int n_viewpoints, const int* view_of, float* normals, float* variation,
                       atvs_stream_t stream);

/* Global registration (ops/cloud.py cloud_fpfh / cloud_feature_nearest / cloud_ransac, atvsnet/register_cloud.py global_init,
 * csrc/cloud_features.hip, csrc/cloud_ransac.hip): FPFH descriptors (Rusu, Blodow and Beetz 2009), their exact nearest neighbour in
 * feature space, and the scoring of three-point hypotheses.  Pointers are device pointers unless named host.  No atomics, no host
 * synchronisation, no allocation, no transcendental function; every operation is rounded on its own, nothing is contracted; the
 * same input gives the same bits on every run.  tests/cloud_global_restated.py restates all three definitions.
 *
 * atvs_cloud_fpfh.  points P (n,3) float32, idx (n,k) int32 = atvs_cloud_knn of the cloud in itself with exclude_same_index
 * (1 <= k <= ATVS_CLOUD_MAX_K; a negative entry is padding), normals N (n,3) float32 = atvs_cloud_normals' (unoriented; a zero row
 * is allowed) -> out (n,33) float32.  Two launches, one lane per point.  Per point j, in double:
 *   a neighbour   t is VALID when 0 <= i = idx[j,t] < n and P[i] is finite; d_t = (double)P[i] - (double)P[j] per component.
 *   the sign      c = sum of d_t over the valid t, from +0 in ascending t (the direction to the neighbours' centroid);
 *                 u = -N[j] when (N_0 c_0 + N_1 c_1) + N_2 c_2 < 0, else N[j] (kept when the dot is 0 or NaN): the normal points
 *                 to the concave side, whatever sign atvs_cloud_normals gave it.  Per neighbour, e = (u_0 m_0 + u_1 m_1) + u_2 m_2
 *                 with m = N[i]; m is negated when e < 0, so that u . m >= 0.
 *   a pair counts when t is valid, N[j] and N[i] are finite with (m_0 m_0 + m_1 m_1) + m_2 m_2 > 0, P[j] is finite,
 *                 dd = (d_0 d_0 + d_1 d_1) + d_2 d_2 > 0, and with g = u x d (g_0 = u_1 d_2 - u_2 d_1, cyclic),
 *                 gg = (g_0 g_0 + g_1 g_1) + g_2 g_2 > 0.
 *   the frame     v = g / sqrt(gg) per component; w = u x v.
 *   the features  alpha = (v_0 m_0 + v_1 m_1) + v_2 m_2;  phi = ((u_0 d_0 + u_1 d_1) + u_2 d_2) / sqrt(dd);
 *                 x = (u_0 m_0 + u_1 m_1) + u_2 m_2 (>= 0 by the sign rule), y = (w_0 m_0 + w_1 m_1) + w_2 m_2, theta = atan2(y, x),
 *                 which the sign rule keeps in [-pi/2, pi/2].
 *   the bins      11 per feature.  alpha: the number of e in 1..10 with 11 alpha >= 2 e - 11 (the edges -9/11 .. 9/11); phi the
 *                 same.  theta: the number of e in 1..10 with C_e y - S_e x >= 0, where (C_e, S_e) = (cos, sin) of the edge
 *                 (2 e - 11) pi / 22, tabulated below; no angle is ever formed.  An exact tie goes to the UPPER bin.
 *   SPFH          33 integer counts h_b (alpha 0..10, phi 11..21, theta 22..32) and the number of counting pairs c_j, kept as 36
 *                 bytes per point (33 counts, c_j, two zero bytes) in scratch: the second launch gathers k x 36 bytes per lane.
 *   FPFH          c_j = 0: the zero row.  Else g_b from +0: for every valid t in ascending order with dd > 0 (recomputed, PCL's
 *                 weight 1 / dd) and c_i > 0: r = 1 / ((double)c_i dd), g_b = g_b + (double)h_b(i) r.
 *   the output    per 11-bin part s = the sum of its g_b from +0 in ascending b; with the point's own f_b = (double)h_b / (double)c_j:
 *                 out_b = (float)((f_b + g_b / s) 0.5), and (float)f_b when s is not > 0 (no neighbour has a histogram).  The
 *                 neighbours' sum is scaled to 1 BEFORE the point's own part joins it (Open3D's order): SPFH(p) + sum SPFH(q) / dd
 *                 as it stands would weigh the two by the cloud's unit of length.  Each part sums to 1, and the descriptor is
 *                 unchanged when the cloud is scaled, moved or turned, and when any normal is negated.
 * scratch: atvs_cloud_fpfh_scratch_size(n) bytes.  n = 0 is valid.  n negative or beyond 2^30, k outside [1, ATVS_CLOUD_MAX_K], a
 * short scratch: ATVS_ERR_SHAPE.
 *
 * atvs_cloud_feature_nearest.  ref (n,33) float32, query (m,33) float32 -> d2 (m) float32, idx (m) int32: per query the smallest
 * d2 = the float32 sum of (q_b - r_b)(q_b - r_b) over b = 0..32, the first product taken as it is, the others added in ascending b,
 * over the reference rows that are not all zero, and the lowest index attaining it.  (+inf, -1) for a query whose 33 entries are
 * all zero, and when no reference row qualifies (a NaN distance never wins).  Exact brute force on the vector unit: reference
 * rows pass through LDS in tiles of ATVS_CLOUD_FEATURE_TILE, each lane owns one query.  n and m up to 2^30; beyond, or negative:
 * ATVS_ERR_SHAPE.  m = 0 is valid.
 *
 * atvs_cloud_ransac_score.  src (c,3) and dst (c,3) float32: row i of one matches row i of the other; triples (h,3) int32; tau > 0,
 * edge_ratio in (0, 1], with_scale 0 or 1, best in 1..ATVS_CLOUD_RANSAC_MAX_BEST -> out, best x 15 8-byte words.  One lane per
 * hypothesis, in double.  With a_k = (double)src[i_k], b_k = (double)dst[i_k] for the triple (i_0, i_1, i_2):
 *   the edges     of each triangle: p = x_1 - x_0, q = x_2 - x_0, r = x_2 - x_1; lengths l_01, l_02, l_12 = sqrt((e_0 e_0 + e_1 e_1) + e_2 e_2).
 *   the frame     X = p / l_01; z = q - ((q_0 X_0 + q_1 X_1) + q_2 X_2) X; zz = (z_0 z_0 + z_1 z_1) + z_2 z_2; Y = z / sqrt(zz);
 *                 Z = X x Y.  R[r][c] = (Xd_r Xs_c + Yd_r Ys_c) + Zd_r Zs_c (d: dst's frame, s: src's): a rotation to rounding.
 *   the scale     s = ((ld_01 + ld_02) + ld_12) / ((ls_01 + ls_02) + ls_12) when with_scale, else 1.
 *   the matrix    M[r][c] = s R[r][c]; with the centroids g = ((x_0 + x_1) + x_2) / 3 per component,
 *                 M[r][3] = gd_r - ((M[r][0] gs_0 + M[r][1] gs_1) + M[r][2] gs_2).
 *   invalid       (count -1) unless all of: 0 <= i_k < c, the three indices differ; every squared edge length of both triangles
 *                 >= ATVS_CLOUD_RANSAC_MIN_EDGE2 (1e-60: the floor that keeps the divisions finite); zz > 1e-12 (q . q) in both
 *                 triangles (the sine of the angle at x_0 above 1e-6: not a zero area); and for each of the three edges
 *                 ld >= edge_ratio (s ls) and edge_ratio ld <= s ls.  Every test is written so that a NaN fails it.
 *   the score     over ALL c pairs in ascending i (the triple's own included): x = (double)src[i];
 *                 e_r = (((M[r][0] x_0 + M[r][1] x_1) + M[r][2] x_2) + M[r][3]) - (double)dst[i]; d = (e_0 e_0 + e_1 e_1) + e_2 e_2; the
 *                 pair counts when d <= tau tau, and the sum takes d in that order from +0.  Pairs pass through LDS in tiles of
 *                 256; every lane reads the same address.
 *   the selection the order is larger count, then smaller sum, then lower index; invalid hypotheses never enter.  One workgroup
 *                 finds the first `best` of that order in `best` rounds, each a fold of the fixed shape of the moments' tree (a
 *                 lane takes lane + 32, + 16, .. + 1; the wavefronts as (w0, w1), (w2, w3)); the order is total, so the answer
 *                 does not depend on the shape.  Slot r of out: M (12 doubles, row-major 3 x 4), the count (int64), the sum
 *                 (double), the hypothesis' index (int64); a slot beyond the number of valid hypotheses: zeros, -1, +0, -1.
 * scratch: atvs_cloud_ransac_scratch_size(h) bytes; afterwards it begins with the h counts (int32, -1 for an invalid hypothesis)
 * and holds the h sums (double) from the next multiple of 256 bytes on.  c in 3..2^30, h in 1..2^24, else ATVS_ERR_SHAPE; tau or
 * edge_ratio outside their range or NaN, with_scale not 0 or 1, best outside its range: ATVS_ERR_ARG. */
#define ATVS_CLOUD_FPFH_BINS 11
#define ATVS_CLOUD_FPFH_THETA_COS { 0.28173255684142978, 0.54064081745559767, 0.75574957435425827, 0.90963199535451844, 0.98982144188093268, 0.98982144188093268, 0.90963199535451844, 0.75574957435425827, 0.54064081745559767, 0.28173255684142978 }
#define ATVS_CLOUD_FPFH_THETA_SIN { -0.95949297361449737, -0.84125353283118109, -0.6548607339452851, -0.41541501300188638, -0.14231483827328514, 0.14231483827328514, 0.41541501300188638, 0.6548607339452851, 0.84125353283118109, 0.95949297361449737 }
#define ATVS_CLOUD_FEATURE_TILE 128
#define ATVS_CLOUD_RANSAC_MAX_BEST 8
#define ATVS_CLOUD_RANSAC_MIN_EDGE2 1e-60
int atvs_cloud_fpfh_scratch_size(long n, long* bytes);
int atvs_cloud_fpfh(const float* points, long n, const int* idx, int k, const float* normals, void* scratch, long scratch_bytes,
                    float* out, atvs_stream_t stream);
int atvs_cloud_feature_nearest(const float* ref, long n, const float* query, long m, float* d2, int* idx, atvs_stream_t stream);
int atvs_cloud_ransac_scratch_size(long h, long* bytes);
int atvs_cloud_ransac_score(const float* src, const float* dst, long c, const int* triples, long h, double tau, int with_scale,
                      double edge_ratio, int best, void* scratch, long scratch_bytes, void* out, atvs_stream_t stream);

/* A scan rendered into cameras (ops/cloud.py scan_render, atvsnet/eval_depth.py, csrc/scan_render.hip): the ground-truth depth
 * maps a set of depth maps is scored against.  Pointers are device pointers.  Integer atomics only: the output is a function of the
 * inputs alone, bit for bit on every run.  No host synchronisation, no allocation; scratch is the caller's.
 * tests/scan_render_restated.py restates the definition.
 *
 * The definition.  points P (n,3) float32 in the cameras' frame; cams (n_cams,16) doubles per camera = R (3x3, row-major, world to
 * camera), t (3), fx, fy, cx, cy; maps of rows x cols pixels.  Per (camera, point), in double, every operation rounded, nothing
 * contracted: c_k = ((R_k0 X + R_k1 Y) + R_k2 Z) + t_k, x = (c_0 / c_2) fx + cx, y = (c_1 / c_2) fy + cy (atvs_colmap_depth_range's
 * projection), xs = (x - pixel_centre) + 0.5, ys = (y - pixel_centre) + 0.5.  pixel_centre is the image coordinate of the centre
 * of pixel (0,0): 0.0 is the convention of the fusion (fusion_pixel.h back-projects integer pixel coordinates), 0.5 the plane
 * sweep's.  The pair takes part when c_2 > 0, z = (float)c_2 is finite and > 0, and xs >= -splat, xs < cols + splat,
 * ys >= -splat, ys < rows + splat (compared in double before any integer conversion; NaN fails).  Then u = (int)floor(xs),
 * v = (int)floor(ys).  Two planes of unsigned 32-bit words per camera, all-ones at first: near[v][u] = min(bits(z)) where (u, v)
 * lies inside the image; front[v + dv][u + du] = min(bits(z)) for every |du|, |dv| <= splat inside the image (a positive float
 * orders as its bits do).  Per pixel: depth = 0 where near is all-ones; otherwise, with z = float(near) and zf = float(front),
 * depth = z when (double)z <= (double)zf * (1.0 + occlusion_tol), else 0 -- a background point seen through a hole of a nearer
 * surface.  With splat = 0 every near pixel survives.  This is a point splat, not a visibility-aware renderer: the scan's own
 * occlusions and holes are not modelled.
 *
 * atvs_scan_render: depth_out (n_cams, rows, cols) float32 as defined.  scratch: atvs_scan_render_scratch_size(n_cams, rows, cols)
 * bytes (the two planes), filled by hipMemsetAsync on the stream.  Two launches (one when n = 0: all-zero maps).
 * splat outside [0, ATVS_SCAN_RENDER_MAX_SPLAT], occlusion_tol negative or not finite, pixel_centre not finite: ATVS_ERR_ARG;
 * n_cams * rows * cols >= 2^31, n_cams outside [1, ATVS_SCAN_RENDER_MAX_CAMS], rows or cols < 1, n negative or beyond 2^30, a short
 * scratch: ATVS_ERR_SHAPE. */
#define ATVS_SCAN_RENDER_MAX_SPLAT 4
#define ATVS_SCAN_RENDER_MAX_CAMS 65535
int atvs_scan_render_scratch_size(int n_cams, int rows, int cols, long* bytes);
int atvs_scan_render(const float* points, long n, const double* cams, int n_cams, int rows, int cols, double pixel_centre, int splat,
                     double occlusion_tol, void* scratch, long scratch_bytes, float* depth_out, atvs_stream_t stream);

/* Scoring a cloud by ETH3D's published protocol, restated (ops/cloud.py cloud_scan_excess / cloud_voxel_shares,
 * atvsnet/eval_cloud.py, csrc/cloud_visibility.hip, csrc/cloud_register.hip): a point's signed distance to what a laser scanner saw
 * along its ray, and per-voxel shares averaged over voxels.  Pointers are device pointers unless marked HOST.  No float atomics, no
 * host synchronisation, no allocation; every output is a function of the inputs alone, bit for bit on every run.
 * tests/cloud_eth3d_restated.py restates both definitions.
 *
 * atvs_cloud_scan_excess.  points (m,3) float32; S = n_scanners >= 1 scanners, 6 S <= ATVS_SCAN_RENDER_MAX_CAMS; cams (6 S,16)
 * doubles in atvs_scan_render's layout, six faces per scanner (a cube map: six 90-degree pinhole cameras at the scanner's origin);
 * maps (6 S, size, size) float32 as atvs_scan_render returns them for those cameras (0 = empty pixel); window w in
 * 0..ATVS_CLOUD_SCAN_MAX_WINDOW.  Per (point, scanner), in double, every operation rounded, nothing contracted: for the faces
 * f = 0..5 in order, c, xs, ys are
 * atvs_scan_render's (csrc/scan_project.h is the one definition both use) and the face is IN VIEW under its rule at splat = 0 with
 * rows = cols = size: c_2 > 0, (float)c_2 finite and > 0, 0 <= xs < size, 0 <= ys < size.  The FIRST face in view is the point's
 * face (the tie rule on cube edges); with none the scanner does not observe the point (its own origin is such a point).
 * u = (int)floor(xs), v = (int)floor(ys); z_scan = the minimum of the non-zero map values at (u + du, v + dv), |du|, |dv| <= w,
 * inside that face -- a window does NOT cross a cube edge into the neighbouring face; with no non-zero value the scanner does not
 * observe the point.  r = sqrt((c_0 c_0 + c_1 c_1) + c_2 c_2), e_s = r * (1.0 - (double)z_scan / c_2): negative = in front of the
 * nearest scan sample along that ray by |e_s| (free space), positive = behind it.  excess (m) float32 = (float)min_s e_s over the
 * observing scanners, scanner (m) int32 = the lowest s attaining the minimum (compared in double); (+inf, -1) when no scanner
 * observes the point or the point is not finite.  One launch; m = 0 writes nothing.
 * w outside [0, ATVS_CLOUD_SCAN_MAX_WINDOW], pixel_centre not finite: ATVS_ERR_ARG; size < 1, S < 1,
 * 6 S > ATVS_SCAN_RENDER_MAX_CAMS, 6 S size size >= 2^31, m negative or beyond 2^30: ATVS_ERR_SHAPE.
 *
 * atvs_cloud_voxel_shares.  points (n,3) float32, d2 (n) float32 of atvs_cloud_nearest, excess (n) float32 of
 * atvs_cloud_scan_excess or NULL, voxel and origin (HOST, 3 finite doubles) as for atvs_cloud_voxel_downsample, tolerances (HOST,
 * 1..ATVS_CLOUD_MAX_TOLERANCES doubles >= 0), margin (a double, not NaN).  A point's voxel is atvs_cloud_voxel_downsample's cell
 * triple (one function in csrc/cloud_register.hip); non-finite points belong to no voxel.  Per voxel and tolerance tau: hit = the
 * number of its points with (double)d2 <= tau * tau; den = all its points when excess is NULL, otherwise hit + the number of
 * points that are not hit and have (double)excess <= margin (the rest -- behind everything a scanner saw, or seen by none -- are
 * UNOBSERVED and count nowhere; a NaN is neither hit nor observed).  A voxel with den = 0 is left out at that tau; otherwise q = (hit * 2^32) / den
 * in unsigned 64-bit integer division.  out (n_tolerances,4) int64: sum of q, the number of voxels counted, sum of hit, sum of
 * den.  The share is sum q / (voxels * 2^32), formed by the caller.  Unsigned integer atomics only.  A finite point whose cell
 * leaves [0, 2^21) on an axis makes the call a shape error that only the device can see: every word of out is -1 (ops/cloud.py
 * raises).  n = 0: zero words.  Tolerances are taken four at a time (count and reduce launches per pass).
 * scratch: atvs_cloud_voxel_shares_scratch_size(n) bytes: 40 B per slot of the table (capacity = the power of two >=
 * max(2 n, 1024)) and 4 B per point: 84 to 164 B per point.  voxel <= 0 or not finite, a non-finite origin, a negative or NaN
 * tolerance, a NaN margin: ATVS_ERR_ARG; n negative or beyond 2^30, n_tolerances outside [1, ATVS_CLOUD_MAX_TOLERANCES], a short
 * scratch: ATVS_ERR_SHAPE. */
#define ATVS_CLOUD_SCAN_MAX_WINDOW 2
int atvs_cloud_scan_excess(const float* points, long m, const double* cams, const float* maps, int n_scanners, int size,
                           double pixel_centre, int window, float* excess, int* scanner, atvs_stream_t stream);
int atvs_cloud_voxel_shares_scratch_size(long n, long* bytes);
int atvs_cloud_voxel_shares(const float* points, const float* d2, const float* excess, long n, double voxel, const double* origin,
                            const double* tolerances, int n_tolerances, double margin, void* scratch, long scratch_bytes,
                            long long* out, atvs_stream_t stream);

/* A surface from depth maps (ops/tsdf.py tsdf_integrate / tsdf_mesh, atvsnet/mesh_fusion.py, csrc/tsdf.hip): a block-sparse
 * truncated-signed-distance (TSDF) volume integrated from depth maps, and a marching-tetrahedra extractor.  Pointers are device
 * pointers unless marked HOST.  No float atomics, no allocation; every output is a function of the inputs alone, bit for bit on
 * every run.  tests/tsdf_restated.py restates both definitions on a dense grid.
 *
 * The box.  origin (HOST, 3 finite doubles), voxel > 0, bx x by x bz blocks of 8^3 voxels, bx by bz <= ATVS_TSDF_MAX_DIRECTORY.
 * Voxel (i, j, k) has its centre at origin[a] + ((double)i_a + 0.5) * voxel, every operation rounded.  A block's linear index is
 * (z by + y) bx + x; inside a block voxels are indexed [z][y][x].
 *
 * Integration.  depths (n, rows, cols) float32 z-depth (0 or non-finite: no sample), cams (n,16) doubles in atvs_scan_render's
 * layout, images (n, rows, cols, channels >= 3) float32 with b, g, r in channels 0..2, or NULL.  Per voxel, views ascending, in
 * double, nothing contracted: the centre is projected by atvs_scan_render's projection (csrc/scan_project.h; in view when c_2 > 0,
 * (float)c_2 finite and > 0, 0 <= xs < cols, 0 <= ys < rows); the pixel is (floor(xs), floor(ys)), d its depth; the view
 * contributes when d > 0, d is finite and sdf = (double)d - c_2 lies in [-trunc, trunc]; then S += sdf / trunc, W += 1,
 * C[c] += (double)image[c].  tsdf = (float)(S / W), weight = (float)W, color[c] = (float)(C[c] / W); all 0 where W = 0.  A view
 * outside the narrow band adds nothing (no free-space carving), so a voxel's values do not depend on which blocks exist.
 *   atvs_tsdf_mark: directory (bx by bz unsigned words) = 1 for every block that the padded box of some pixel's frustum segment
 *   [d - trunc, d + trunc] meets, 0 elsewhere -- a superset of the blocks with a contributing voxel; err (one int) = 1 when a
 *   pixel's box meets more than ATVS_TSDF_MAX_PIXEL_BLOCKS blocks (the voxel is too small for these maps), else 0.
 *   atvs_tsdf_scan: counters (count unsigned words) -> their exclusive prefix sum in place, total[0] (device, 64-bit) = their sum.
 *   scratch: atvs_tsdf_scan_scratch_size(count) bytes.  count = 0 writes total alone.  count beyond 2^31: ATVS_ERR_SHAPE.
 *   atvs_tsdf_assign: slots = the scanned directory, count its total -> coords (count,3) int32 (x, y, z of each slot's block,
 *   ascending in the linear index) and masks (count, ceil(n / 64)) 64-bit words: bit v of a slot is set when a pixel of view v
 *   marked the block.
 *   atvs_tsdf_integrate: one workgroup per slot over the views of its mask -> tsdf, weight (count,8,8,8), color (count,8,8,8,3) or
 *   NULL with images NULL, any (count unsigned words) = 1 where the slot has a voxel of weight > 0.
 *   atvs_tsdf_gather: keep = the scanned `any`, kept its total -> the kept slots, in order, in coords_out, tsdf_out, weight_out,
 *   color_out: exactly the blocks that have a voxel of weight > 0; free_in (count,8,8,8) or NULL is carried into free_out alike.
 * trunc <= 0 or not finite, voxel <= 0 or not finite, a non-finite origin or pixel_centre: ATVS_ERR_ARG; n rows cols >= 2^31,
 * n outside [1, ATVS_SCAN_RENDER_MAX_CAMS], a box beyond the limit, count beyond the directory, channels < 3: ATVS_ERR_SHAPE.
 *
 * Free-space carving (opt-in: atvs_tsdf_integrate_carve; atvs_tsdf_integrate is as above).  Per voxel and view, views ascending,
 * in double, nothing contracted, with exactly the projection and the pixel above: d is the pixel's depth, sdf = (double)d - c_2.
 * A view that is in view (scan_project true) with d > 0 and d finite is IN BAND when -trunc <= sdf <= trunc -- the contribution to
 * S, W, C above, unchanged and in the same order --, FREE when sdf > trunc: Wf += 1, no colour (the view saw past the voxel), and
 * nothing when sdf < -trunc (the voxel is occluded).  A depth that is no sample (0, negative, NaN, +-inf) carves nothing; a voxel
 * behind the camera (c_2 <= 0) or outside the image is not carved.  At the end, with cw = carve_weight > 0 and f = cw * Wf formed
 * once: weight = (float)W (the in-band count only: min_weight keeps its meaning), free = (float)Wf where W > 0, else 0,
 * tsdf = (float)((S + f) / (W + f)) where W > 0, else 0, colour as above.  The volume holds exactly the blocks with a voxel of
 * W > 0: a voxel that no view has in band is not carved, so the values still do not depend on which blocks or views an
 * implementation visits.  Consequences: blocks, weight and color are bit for bit those of the run without carving, and so is tsdf
 * wherever free == 0 (f = 0, and S is never -0: d - c_2 rounds an exact zero to +0).
 *   atvs_tsdf_free_views: coords (count,3) int32 block coordinates -> masks (count, ceil(n / 64)) 64-bit words: bit v is set unless
 *   view v provably sees no voxel centre of the block.  The rule, exactly: the eight corners of the block's cube are
 *   origin[a] + (double)(8 * (b[a] + delta_a)) * voxel, delta in {0,1}^3; for each, c_2, then c_0, c_1, x, y, xs, ys in
 *   scan_project's operation order.  No corner has c_2 > 0: clear.  Some corners have c_2 > 0 and some do not, or xs or ys of a
 *   corner with c_2 > 0 is NaN: set.  All eight have c_2 > 0: set iff max xs >= -1, min xs < cols + 1, max ys >= -1 and
 *   min ys < rows + 1.  With c_2 > 0 over the whole cube its image lies in the hull of the corners' images, so the mask is a
 *   superset of the views that contribute to or carve a voxel of the block; the pixel of padding is far above the rounding of the
 *   corner arithmetic.  Depths are not consulted.  The bits of the last word beyond view n - 1 are 0.
 *   atvs_tsdf_integrate_carve: as atvs_tsdf_integrate over the views of masks | free_masks (both (count, ceil(n / 64))), with
 *   free_out (count,8,8,8).  carve_weight <= 0 or not finite: ATVS_ERR_ARG.
 *
 * Per-pixel view weights (opt-in: atvs_tsdf_integrate_weighted; the two entry points above are as they were).  weights (n, rows,
 * cols) float32 beside depths.  Per voxel and view, views ascending, in double, nothing contracted, with exactly the projection and
 * the pixel above: d is the pixel's depth, w the pixel's weight.  The view is a SAMPLE only when the conditions above hold (in
 * view, d > 0, d finite) and w > 0 and w is finite; a weight that is 0, negative, NaN or infinite makes the view no sample at that
 * pixel: it neither contributes nor carves.  A sample in band (-trunc <= sdf <= trunc) adds S += (double)w * (sdf / trunc),
 * W += (double)w, C[c] += (double)w * (double)image[c], each product rounded before its sum; with carving a free sample
 * (sdf > trunc) adds Wf += (double)w.  The epilogues are the ones above, unchanged: tsdf = (float)(S / W) without carving,
 * (float)((S + f) / (W + f)) with f = cw * Wf formed once with it; weight = (float)W, now a sum of weights, which
 * atvs_tsdf_mesh_count's min_weight is compared with as before; free = (float)Wf where W > 0; color[c] = (float)(C[c] / W); all 0
 * where W = 0.  Marking and assignment read the depths alone and are untouched: a marked block whose samples all have a weight that
 * is no weight ends with W = 0 everywhere and is dropped by atvs_tsdf_gather, so the volume still holds exactly the blocks with a
 * voxel of W > 0.  Consequences: with every weight 1.0 each array is bit for bit the one of the call without weights, with and
 * without carving (1.0 * x is exact, the sums run in the same order); with weights that are 0 where a mask is false and 1 elsewhere
 * the volume is the one integrated from the depths zeroed by that mask.
 *   atvs_tsdf_integrate_weighted: as atvs_tsdf_integrate_carve with weights after depths.  free_masks and free_out may both be
 *   NULL: no carving, the views of masks alone, carve_weight is not read.  One of the two NULL: ATVS_ERR_NULL.  weights NULL:
 *   ATVS_ERR_NULL.  With carving carve_weight <= 0 or not finite: ATVS_ERR_ARG.
 *
 * Extraction.  blocks (nb,3) int32 ascending in the linear index, each at most once, nb <= ATVS_TSDF_MAX_MESH_BLOCKS; tsdf, weight
 * (nb,8,8,8), color (nb,8,8,8,3) or NULL.  A voxel is VALID when weight >= min_weight (a voxel of a missing block or outside the
 * box is not); INSIDE means tsdf < 0.  The cube of voxel (i, j, k) has the 8 centres (i..i+1, j..j+1, k..k+1) and is meshed when
 * all 8 are valid.  Its six Kuhn tetrahedra are taken in the lexicographic order of the axis permutations; for (a, b, c) the local
 * vertices are 0 = corner 000, 1 = +e_a, 2 = +e_a + e_b, 3 = corner 111.  One local vertex s on one side: the triangle over the
 * edges (s, o_0), (s, o_1), (s, o_2), the others ascending.  Two and two, inside {a < b}, outside {c < d}: (ac, ad, bd), then
 * (ac, bd, bc).  A triangle's last two vertices are swapped when its normal, with every crossing at its edge's midpoint, points
 * against (centroid of the outside corners - centroid of the inside corners): normals point into free space.  Then it is rotated
 * so that its smallest vertex index comes first.  A vertex lives on an edge, owned by the edge's lower voxel; the seven edge types
 * are the offsets (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1).  An edge has a vertex when its endpoints differ in
 * INSIDE and a meshed cube has both among its corners.  With fa, fb the endpoints' tsdf as doubles: t = fa / (fa - fb),
 * p = pa + t * (pb - pa) per coordinate in double, cast to float32; colour = floor((ca + t * (cb - ca)) + 0.5) clamped to 0..255,
 * stored r, g, b.  Vertices are ordered by owning voxel (blocks ascending, x fastest inside a block), then edge type; faces by
 * cube in that order, then tetrahedron, then the two triangles.  Zero-area triangles (tsdf == 0 at a corner) are kept.
 * Special values follow from these comparisons as written and from nothing else.  VALID is the comparison weight >= min_weight in
 * float32: a NaN weight is never valid, a +inf weight is valid under every min_weight, min_weight = -inf makes every voxel of a
 * present block valid (one of a missing block stays invalid).  INSIDE is the comparison tsdf < 0: +0, -0, a positive denormal, +inf
 * and a NaN are outside, a negative denormal and -inf are inside.  t, p and the colour expression are plain IEEE double arithmetic,
 * so a NaN or an infinite tsdf or colour goes through them as it does (inf / inf and 0 * inf are NaN; a vertex coordinate may be
 * NaN, its sign and payload unspecified).  A colour is v = floor(x + 0.5), then 0 unless v >= 0, then 255 unless v <= 255: NaN and
 * -inf give 0, +inf gives 255.
 *   atvs_tsdf_mesh_count: cube_ok, emask (nb 512 bytes each), vcount, fcount (nb 512 unsigned words each): per voxel whether its
 *   cube is meshed, the set of its edge types that carry a vertex, their number, its cube's triangles.
 *   atvs_tsdf_mesh_emit: vstart, fstart = vcount, fcount after atvs_tsdf_scan, n_vertices, n_faces their totals -> vertices
 *   (n_vertices,3) float32, colors (n_vertices,3) bytes or NULL with color NULL, faces (n_faces,3) int32.
 * A NaN min_weight: ATVS_ERR_ARG; nb negative, beyond the limit or the box: ATVS_ERR_SHAPE. */
#define ATVS_TSDF_MAX_DIRECTORY 67108864
#define ATVS_TSDF_MAX_MESH_BLOCKS 262144
#define ATVS_TSDF_MAX_PIXEL_BLOCKS 4096
int atvs_tsdf_scan_scratch_size(long count, long* bytes);
int atvs_tsdf_scan(void* counters, long count, void* scratch, long scratch_bytes, long long* total, atvs_stream_t stream);
int atvs_tsdf_mark(const float* depths, const double* cams, int n, int rows, int cols, double voxel, double trunc,
                   const double* origin, int bx, int by, int bz, double pixel_centre, void* directory, int* err,
                   atvs_stream_t stream);
int atvs_tsdf_assign(const float* depths, const double* cams, int n, int rows, int cols, double voxel, double trunc,
                     const double* origin, int bx, int by, int bz, double pixel_centre, const void* slots, long count, int* coords,
                     void* masks, int* err, atvs_stream_t stream);
int atvs_tsdf_integrate(const float* depths, const float* images, int channels, const double* cams, int n, int rows, int cols,
                        double voxel, double trunc, const double* origin, int bx, int by, int bz, double pixel_centre,
                        const int* coords, const void* masks, long count, float* tsdf, float* weight, float* color, void* any,
                        atvs_stream_t stream);
int atvs_tsdf_gather(const int* coords, const float* tsdf, const float* weight, const float* color, const void* keep, long count,
                     long kept, int* coords_out, float* tsdf_out, float* weight_out, float* color_out, const float* free_in,
                     float* free_out, atvs_stream_t stream);
int atvs_tsdf_free_views(const int* coords, long count, const double* cams, int n, int rows, int cols, double voxel,
                         const double* origin, int bx, int by, int bz, double pixel_centre, void* masks, atvs_stream_t stream);
int atvs_tsdf_integrate_carve(const float* depths, const float* images, int channels, const double* cams, int n, int rows, int cols,
                              double voxel, double trunc, const double* origin, int bx, int by, int bz, double pixel_centre,
                              const int* coords, const void* masks, const void* free_masks, double carve_weight, long count,
                              float* tsdf, float* weight, float* color, float* free_out, void* any, atvs_stream_t stream);
int atvs_tsdf_integrate_weighted(const float* depths, const float* weights, const float* images, int channels, const double* cams,
                                 int n, int rows, int cols, double voxel, double trunc, const double* origin, int bx, int by, int bz,
                                 double pixel_centre, const int* coords, const void* masks, const void* free_masks,
                                 double carve_weight, long count, float* tsdf, float* weight, float* color, float* free_out,
                                 void* any, atvs_stream_t stream);
int atvs_tsdf_mesh_count(const int* blocks, int nb, int bx, int by, int bz, const float* tsdf, const float* weight,
                         float min_weight, void* cube_ok, void* emask, void* vcount, void* fcount, atvs_stream_t stream);
int atvs_tsdf_mesh_emit(const int* blocks, int nb, int bx, int by, int bz, double voxel, const double* origin, const float* tsdf,
                        const float* color, const void* emask, const void* vstart, const void* fstart, long n_vertices,
                        long n_faces, float* vertices, void* colors, int* faces, atvs_stream_t stream);

/* A triangle mesh rendered into cameras (ops/mesh.py mesh_render / depth_occlude, atvsnet/eval_depth.py, csrc/mesh_render.hip):
 * per pixel the nearest depth of the mesh along the ray through the pixel's centre, and the face that gives it.  Pointers are
 * device pointers.  A 64-bit integer atomic min and no float atomics: the outputs are a function of the inputs alone, bit for bit
 * on every run.  No host synchronisation, no allocation; scratch is the caller's.  tests/mesh_render_restated.py restates the
 * definition densely (every face against every pixel).
 *
 * The definition.  vertices (n_vertices,3) float32 in the cameras' frame, faces (n_faces,3) int32 indices into them, cams
 * (n_cams,16) doubles in atvs_scan_render's layout (c = R row-major, t, fx, fy, cx, cy), maps of rows x cols pixels.  Everything
 * in double, every operation rounded, nothing contracted, in exactly this order.
 *   Camera-space vertices.  For a vertex (X, Y, Z) widened to double: C_k = ((c[3k] X + c[3k+1] Y) + c[3k+2] Z) + c[9+k],
 *   k = 0, 1, 2 (atvs_scan_render's form).
 *   Which faces take part.  A face (i0, i1, i2) with camera-space vertices A, B, D takes part in a camera when all nine
 *   coordinates are finite and at least one of A_2, B_2, D_2 is > 0.
 *   Cross products.  N0 = B x D, N1 = D x A, N2 = A x B, a component of a x b being a_1 b_2 - a_2 b_1 (and cyclic): two rounded
 *   products and one subtraction.
 *   Determinant.  det = (A_0 N0_0 + A_1 N0_1) + A_2 N0_2.
 *   Pixel ray.  For pixel (u, v): rx = (((double)u + pixel_centre) - cx) / fx, ry = (((double)v + pixel_centre) - cy) / fy: the
 *   centre of pixel u is the image coordinate u + pixel_centre, the convention under which atvs_scan_render sends x to
 *   floor((x - pixel_centre) + 0.5).
 *   Edge functions.  E_i = (Ni_0 rx + Ni_1 ry) + Ni_2, S = (E0 + E1) + E2.
 *   Coverage.  The pixel is covered when (E0 >= 0 and E1 >= 0 and E2 >= 0 and S > 0) or (E0 <= 0 and E1 <= 0 and E2 <= 0 and
 *   S < 0): both windings, both sides of every edge inclusive, no fill rule, no back-face culling.
 *   Depth.  t = det / S, the camera depth of the point where the ray meets the face's plane (the ray's third component is 1).
 *   The pixel takes part when t > 0 and z = (float)t is finite and > 0.
 *   Per pixel.  The smallest key ((uint64)bits(z) << 32) | face index over the covered faces that take part: a positive float32
 *   orders as its bits do, and on equal z the lower face index wins.  depth_out (n_cams, rows, cols) float32 = that z, 0 where
 *   nothing is covered; face_out (n_cams, rows, cols) int32 = that face, -1 where nothing is covered.
 * No near-plane clipping exists: a face with vertices behind the camera renders where it is in front.  a x b and b x a negate
 * exactly, so the two faces of a shared edge get E and -E at every pixel centre: a closed mesh has no cracks.  Zero-area,
 * edge-on (S = 0), repeated-index, NaN and infinite faces cover nothing.
 *
 * atvs_mesh_render.  A face with an index outside 0..n_vertices-1 is skipped; error_out (one int) = the number of such faces
 * (0: none).  scratch: atvs_mesh_render_scratch_size(n_cams, rows, cols, n_faces) bytes: 8 per pixel and 12 per entry of a list
 * of at most 2^22 (face, camera) pairs whose box holds more than ATVS_MESH_RENDER_SMALL_PIXELS pixels; the faces are walked in
 * chunks that cannot fill the list, so no pair is dropped.  n_faces = 0: all-zero depth, all -1 faces.
 * pixel_centre not finite: ATVS_ERR_ARG; n_cams * rows * cols >= 2^31, n_cams outside [1, ATVS_SCAN_RENDER_MAX_CAMS], rows or
 * cols < 1, n_vertices negative or beyond 2^30, n_faces negative or 2^31 and more, a short scratch: ATVS_ERR_SHAPE.
 *
 * atvs_depth_occlude.  depth, occluder, out: `pixels` float32 each.  out = 0 where occluder > 0 and depth > 0 and
 * !((double)depth <= (double)occluder * (1.0 + tol)), else out = depth: a NaN in either keeps depth.  out may be depth (in place).
 * One launch; pixels = 0 writes nothing.  tol negative or not finite: ATVS_ERR_ARG; pixels negative or 2^31 and more:
 * ATVS_ERR_SHAPE. */
#define ATVS_MESH_RENDER_SMALL_PIXELS 64
int atvs_mesh_render_scratch_size(int n_cams, int rows, int cols, long n_faces, long* bytes);
int atvs_mesh_render(const float* vertices, long n_vertices, const int* faces, long n_faces, const double* cams, int n_cams, int rows,
                     int cols, double pixel_centre, void* scratch, long scratch_bytes, float* depth_out, int* face_out,
                     int* error_out, atvs_stream_t stream);
int atvs_depth_occlude(const float* depth, const float* occluder, long pixels, double tol, float* out, atvs_stream_t stream);

/* The connectivity of a triangle mesh (ops/mesh_topology.py, atvsnet/clean_mesh.py, csrc/mesh_topology.hip): connected components,
 * the selection of faces, the edge census.  Pointers are device pointers.  Integer arithmetic and integer atomics only, no float
 * atomics: the outputs are a function of the inputs alone, bit for bit on every run.  No host synchronisation, no allocation;
 * scratch is the caller's.  tests/mesh_topology_restated.py restates the definitions in numpy.  faces (n_faces,3) int32 index
 * n_vertices vertices; n_vertices in 0..2^30 (the limit of atvs_mesh_render), n_faces in 0..ATVS_MESH_TOPOLOGY_MAX_FACES, anything
 * else ATVS_ERR_SHAPE, as is a short scratch; a null pointer that is needed ATVS_ERR_NULL; both without a launch.
 *
 * atvs_mesh_components.  Two vertices are connected when one face names both; a component is a class of the transitive closure.  A
 * face with repeated indices still connects what it names.  vertex_component (n_vertices,) int32: -1 for a vertex no face names,
 * else the dense id of its component, ids 0..C-1 in ascending order of the component's smallest vertex index.  face_component
 * (n_faces,) int32: the component of the face's first vertex.  face_count and vertex_count: max(1, min(n_vertices, n_faces)) int32
 * each (a component has a face and a vertex of its own, so C is no more), the first C the components' faces and vertices, the
 * rest 0.  info: two int32, info[0] = the number of faces with an index outside 0..n_vertices-1 (such a face is skipped, and no
 * output is defined unless it is 0), info[1] = C.  scratch: atvs_mesh_components_scratch_size bytes, 12 per vertex and the scan's
 * tile sums.  n_faces = 0: C = 0 and every vertex_component is -1.
 *
 * atvs_mesh_select.  vertices (n_vertices,3) float32, colors (n_vertices,3) uint8 or null, keep (n_faces,) uint8.  The faces with
 * keep != 0 are kept in their order, the vertices they name are kept in their order, the faces are renumbered.  vertices_out
 * (n_vertices,3), colors_out (n_vertices,3; unused with colors null), faces_out (n_faces,3): the first V' and F' rows are written;
 * coordinates and colours are copied as bits.  vertex_map (n_vertices,) int32: the new index of an old vertex, or -1.  info: three
 * int32, info[0] = the number of KEPT faces with an index outside 0..n_vertices-1 (no output is defined unless it is 0), info[1] =
 * V', info[2] = F'.  scratch: atvs_mesh_select_scratch_size bytes, 4 per vertex and per face and the scan's tile sums.
 *
 * atvs_mesh_edge_census.  Each of the 3 n_faces pairs (f0,f1), (f1,f2), (f2,f0) sorted into (lo, hi); pairs with lo == hi count
 * too.  A distinct pair's `faces` is the number of the 3 n_faces pairs that equal it (a face (a,a,a) gives its pair (a,a) three).
 * census: eight int64 words --
 *   [0] edges               the distinct pairs
 *   [1] boundary            distinct pairs with faces == 1
 *   [2] manifold            distinct pairs with faces == 2
 *   [3] nonmanifold         distinct pairs with faces > 2
 *   [4] misoriented         distinct pairs given twice or more in one direction: as (lo,hi) (a pair with lo == hi is given so), or
 *                           as (hi,lo).  0 on a consistently oriented manifold mesh
 *   [5] max_faces_per_edge  the largest faces of a distinct pair
 *   [6] self_edges          distinct pairs with lo == hi
 *   [7] error               faces with an index outside 0..n_vertices-1 (skipped; the other words are defined only when it is 0)
 * scratch: atvs_mesh_edge_census_scratch_size bytes: an open-addressing table of the smallest power of two of slots that is at
 * least 6 n_faces and at least ATVS_MESH_CENSUS_MIN_SLOTS, 16 bytes each (a 64-bit key (lo << 32) | hi and two 32-bit counters):
 * the load is at most 0.5.  ATVS_MESH_TOPOLOGY_MAX_FACES keeps that size in a long.  The probe loop is bounded by the table; a pair
 * that found no slot (impossible at that load) adds to [7].  n_faces = 0: all words 0. */
#define ATVS_MESH_TOPOLOGY_MAX_FACES 268435456
#define ATVS_MESH_CENSUS_MIN_SLOTS 1024
int atvs_mesh_components_scratch_size(long n_vertices, long n_faces, long* bytes);
int atvs_mesh_components(const int* faces, long n_faces, long n_vertices, void* scratch, long scratch_bytes, int* vertex_component,
                         int* face_component, int* face_count, int* vertex_count, int* info, atvs_stream_t stream);
int atvs_mesh_select_scratch_size(long n_vertices, long n_faces, long* bytes);
int atvs_mesh_select(const float* vertices, const void* colors, long n_vertices, const int* faces, const void* keep, long n_faces,
                     void* scratch, long scratch_bytes, float* vertices_out, void* colors_out, int* faces_out, int* vertex_map,
                     int* info, atvs_stream_t stream);
int atvs_mesh_edge_census_scratch_size(long n_faces, long* bytes);
int atvs_mesh_edge_census(const int* faces, long n_faces, long n_vertices, void* scratch, long scratch_bytes, long* census,
                          atvs_stream_t stream);

/* A triangle mesh simplified by vertex clustering (Rossignac and Borrel) with each cluster's representative placed by its quadric
 * (Lindstrom): ops/mesh_simplify.py, atvsnet/simplify_mesh.py, csrc/mesh_simplify.hip; DESIGN.md section 10.3d.  Pointers are device
 * pointers except origin (HOST, 3 finite doubles).  Integer atomics only, no float atomics: every output is a function of the inputs
 * alone, bit for bit on every run.  No host synchronisation, no allocation; scratch is the caller's.
 * tests/mesh_simplify_restated.py restates the definitions in numpy.  vertices (n_vertices,3) float32, colors (n_vertices,3) uint8 or
 * null, faces (n_faces,3) int32, cell a double > 0 (else, or with an origin that is not finite, ATVS_ERR_ARG); n_vertices in 0..2^30,
 * n_faces in 0..ATVS_MESH_TOPOLOGY_MAX_FACES, anything else ATVS_ERR_SHAPE, as is a short scratch; a null pointer that is needed
 * ATVS_ERR_NULL; all without a launch.
 *
 * atvs_mesh_cluster.  The clusters are atvs_cloud_voxel_downsample's voxels: per axis, in double, g = ((double)x - origin) / cell,
 * c = floor(g), u = (uint64)floor((g - c) 2^32) clamped to 2^32 - 1.  A cluster is a triple c; ids 0..C-1 in ascending order of the
 * cluster's lowest vertex index.  vertex_cluster (n_vertices,) int32: the id, -1 for a vertex with a non-finite coordinate (it forms
 * no cluster).  All finite vertices count, whether a face names them or not.  Per cluster, in rows of buffers of n_vertices rows of
 * which the first C are written: cells (.,3) int32 the triple c, counts (.,) int32 the number k of its vertices, position_sums (.,3)
 * the exact unsigned 64-bit sums of u, color_sums (.,3) the integer sums of the colours (not written with colors null).  count: one
 * int64, C -- or -1 when a finite vertex's c leaves [0, 2^21) (no other output is defined then).  scratch:
 * atvs_mesh_cluster_scratch_size(n_vertices) bytes: a table of the smallest power of two of slots that is at least 2 n_vertices and
 * at least 1024, 64 bytes each, and 8 bytes per vertex.
 *
 * atvs_mesh_cluster_quadrics.  quadrics (n_clusters,10) int64 and incidences (n_clusters,) int32, both zeroed here.  A face
 * contributes only if its three vertices are finite (vertex_cluster >= 0) and m = (b - a) x (c - a) has L2 = m.m > 0 and finite;
 * differences are of (double) coordinates, products then additions, (m0 m0 + m1 m1) + m2 m2.  For such a face n = m / sqrt(L2) and
 * w = min(1, sqrt(L2) / (cell cell)): area weighting that saturates for a triangle larger than a cell, which keeps every term in
 * [-1, 1].  The face contributes once to each DISTINCT cluster K among its three: with the face's first vertex (in a, b, c order)
 * that lies in K, p = (g - c) - 0.5 per axis (cell units about the cell's centre), d = -((n0 p0 + n1 p1) + n2 p2), the ten terms
 * w n0 n0, w n0 n1, w n0 n2, w n1 n1, w n1 n2, w n2 n2, w d n0, w d n1, w d n2, w d d -- each ((w x) y) -- are rounded to integers as
 * rint(term 2^30) and added with 64-bit integer atomics; incidences[K] += 1.  At most 3 x 2^28 incidences: no sum reaches 2^60.
 * Zero-area faces and faces with repeated indices add nothing (L2 = 0).  info: one int32, the number of faces with an index outside
 * 0..n_vertices-1 or a vertex_cluster outside -1..n_clusters-1 (skipped; no output is defined unless it is 0).
 *
 * atvs_mesh_cluster_place.  One lane per cluster, everything in double, in cell units about the cell's centre.  The sums are INPUTS
 * (cells, counts, position_sums, color_sums or null, quadrics; quadrics may be null with placement 0).  x0_a = ((double)S_a /
 * (double)k) / 2^32 - 0.5, the exact mean.  placement ATVS_MESH_PLACE_MEAN ends there.  ATVS_MESH_PLACE_QUADRIC: A (symmetric, from
 * sums 0..5) and b (sums 6..8) are (double)sum x 2^-30; A is eigen-decomposed by the fixed 18-rotation Jacobi of atvs_cloud_normals
 * (csrc/jacobi3.h), eigenvalue i on the diagonal and its vector in column i; lambda_max is the largest of the three;
 * g_a = ((A_a0 x0_0 + A_a1 x0_1) + A_a2 x0_2) + b_a; then for i = 0, 1, 2 in turn, where lambda_i > rank_epsilon lambda_max,
 * t = ((v_0i g_0 + v_1i g_1) + v_2i g_2) / lambda_i and x_a = x_a - v_ai t (x starts at x0).  The cluster falls back to x0 when
 * lambda_max <= 2^-20 (a cluster of slivers only), a value is not finite, or any |x_a| > 0.5 (the minimiser leaves the cell:
 * Lindstrom's rule).  positions (n_clusters,3) float32: origin_a + cell (((double)c_a + 0.5) + x_a), rounded once.  colors_out
 * (n_clusters,3) uint8 (with color_sums): (2 S + k) / (2 k) in integers.  placed (n_clusters,) uint8: 1 where the quadric position
 * was used.  rank_epsilon: a double in (0, 1) (else ATVS_ERR_ARG); 1e-3 is Lindstrom's value, a default and not a measurement.  Both
 * placements keep a representative inside its cell, so no vertex moves farther than cell sqrt(3).
 *     The solve's allowance: the Jacobi commits a backward error of at most 128 units of 2^-53 |A| (atvs_cloud_normals' S); on the
 * kept eigenpairs the inverse is at most 1 / (rank_epsilon lambda_max), and |x - x0| <= sqrt(3) inside the cell, so the
 * decomposition moves x by at most 128 sqrt(3) < 222 units of 2^-53 / rank_epsilon.  g costs 6 roundings per row on terms of at most
 * |A| |x0| + |b| <= (0.87 + 3 x 0.87) lambda_max (|b| <= trace(A) sqrt(3) / 2): under 21 units; the three projections and updates
 * (5 + 1 + 2 roundings each on |g| / lambda_i) add under 8 x 3 x 3.5 = 84 more.  Under 327 in all; the header states
 * ATVS_MESH_SIMPLIFY_SOLVE_UNITS = 512 units of 2^-53 / rank_epsilon, in cell units: 5.7e-11 cells at 1e-3, against 9.3e-10 = 2^-30.
 *
 * atvs_mesh_cluster_max_move.  out: one uint32, zeroed here, then the integer atomic max over the finite vertices of the bits of
 * (float)((e0 e0 + e1 e1) + e2 e2), e_a = (double)positions[vertex_cluster][a] - (double)vertices[a] (a non-negative float's bits
 * order as its value): the largest squared move.
 *
 * atvs_mesh_cluster_faces.  faces_out (n_faces,3) int32: a face rewritten to its three cluster ids (-1 for a non-finite vertex;
 * -1, -1, -1 for a face counted in info[0]).  keep (n_faces,) uint8: 0 when the face names a non-finite vertex (info[1],
 * nonfinite_faces), else when two ids are equal (info[2], degenerate_faces), else when a face with a lower index that got this far
 * has the same SET of three ids (info[3], duplicate_faces): the lowest index of each set stays, with its own winding; else 1.
 * info: four int32; info[0] = faces with an index outside 0..n_vertices-1 plus faces that found no slot (impossible at the table's
 * load); no output is defined unless it is 0.  scratch: atvs_mesh_cluster_faces_scratch_size(n_faces) bytes: an open-addressing
 * table of the smallest power of two of slots that is at least 2 n_faces and at least ATVS_MESH_SIMPLIFY_MIN_SLOTS, 4 bytes each (a
 * slot holds a face index; load at most 0.5; every probe loop is bounded by the table), and 4 bytes per face.  atvs_mesh_select
 * then compacts positions and faces_out by keep: surviving faces keep their order and surviving clusters theirs. */
#define ATVS_MESH_SIMPLIFY_MIN_SLOTS 1024
#define ATVS_MESH_SIMPLIFY_SOLVE_UNITS 512
#define ATVS_MESH_PLACE_MEAN 0
#define ATVS_MESH_PLACE_QUADRIC 1
int atvs_mesh_cluster_scratch_size(long n_vertices, long* bytes);
int atvs_mesh_cluster(const float* vertices, const void* colors, long n_vertices, double cell, const double* origin, void* scratch,
                      long scratch_bytes, int* vertex_cluster, int* cells, int* counts, long* position_sums, long* color_sums,
                      long* count, atvs_stream_t stream);
int atvs_mesh_cluster_quadrics(const float* vertices, long n_vertices, const int* faces, long n_faces, const int* vertex_cluster,
                               long n_clusters, double cell, const double* origin, long* quadrics, int* incidences, int* info,
                               atvs_stream_t stream);
int atvs_mesh_cluster_place(const int* cells, const int* counts, const long* position_sums, const long* color_sums,
                            const long* quadrics, long n_clusters, double cell, const double* origin, int placement,
                            double rank_epsilon, float* positions, void* colors_out, void* placed, atvs_stream_t stream);
int atvs_mesh_cluster_max_move(const float* vertices, long n_vertices, const int* vertex_cluster, const float* positions,
                               long n_clusters, void* out, atvs_stream_t stream);
int atvs_mesh_cluster_faces_scratch_size(long n_faces, long* bytes);
int atvs_mesh_cluster_faces(const int* faces, long n_faces, long n_vertices, const int* vertex_cluster, void* scratch,
                            long scratch_bytes, int* faces_out, void* keep, int* info, atvs_stream_t stream);

/* A triangle mesh's surface sampled uniformly by area, so that a mesh scores as a surface and not as its vertices: ops/mesh_sample.py,
 * atvsnet/sample_mesh.py, atvsnet/eval_cloud.py --sample_recon, csrc/mesh_sample.hip; DESIGN.md section 10.3e.  Pointers are device
 * pointers.  Every output is a function of (vertices, colors, faces, density, seed) alone: the random numbers are a hash of (seed,
 * face, sample within the face), the only atomics are integer ones (a sum, a maximum, two tallies), so neither the launch shape nor
 * the order of arrival shows, bit for bit on every run.  No host synchronisation, no allocation; scratch is the caller's.
 * tests/mesh_sample_restated.py restates the definitions in numpy.  vertices (n_vertices,3) float32, colors (n_vertices,3) uint8 or
 * null, faces (n_faces,3) int32; n_vertices in 0..2^30, n_faces in 0..ATVS_MESH_TOPOLOGY_MAX_FACES, n_samples in
 * 0..ATVS_MESH_SAMPLE_MAX, anything else ATVS_ERR_SHAPE, as is a short scratch; density a finite double > 0 (samples per unit area)
 * and seed in 0..2^63-1, else ATVS_ERR_ARG; a null pointer that is needed ATVS_ERR_NULL; all without a launch.
 *
 * The hash.  All arithmetic mod 2^64.  mix(z): z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9, z = (z ^ (z >> 27)) 0x94D049BB133111EB,
 * z ^ (z >> 31) (the finaliser of splitmix64); G = 0x9E3779B97F4A7C15; hash(base, i) = mix(base + G (i + 1)).  The key of face f is
 * k_f = hash(seed, f); sample j of face f draws w = hash(k_f, j).
 *
 * atvs_mesh_sample_counts.  One lane per face, in double: a, b, c the face's vertices, e1 = b - a, e2 = c - a, n = e1 x e2 (products
 * then one subtraction per component), area = 0.5 sqrt((nx nx + ny ny) + nz nz), x = area density,
 * u_f = ((double)(k_f >> 11) + 0.5) 2^-53, count = floor(x) + (u_f < x - floor(x)): stochastic rounding, so a surface of faces with
 * x < 1 still gets its share and the expected count of every face is x.  counts (n_faces,) uint32, areas (n_faces,) float64.  A face
 * with an index outside 0..n_vertices-1 (info[1]) or, else, an area that is not finite (info[2]) is skipped: count 0, area 0.  info:
 * four int64 words, zeroed here: [0] the total of the counts (a 64-bit integer atomic), [1] and [2] the skipped faces, [3] the
 * largest count.  A face with x >= ATVS_MESH_SAMPLE_MAX adds floor(min(x, 2^32)) to [0] and [3] without the rounding bit and its
 * count is not defined; the caller treats info[3] >= ATVS_MESH_SAMPLE_MAX or info[0] > ATVS_MESH_SAMPLE_MAX as a shape error that
 * reports info[0], the samples the density needs, and reads no other output.
 *
 * atvs_mesh_sample_offsets.  offsets (n_faces + 1,) uint32: the exclusive prefix sum of counts (an INPUT here: anybody's counts
 * whose total is at most ATVS_MESH_SAMPLE_MAX), by the point-cloud kernels' scan; offsets[n_faces] is the total.  scratch:
 * atvs_mesh_sample_scratch_size(n_faces) bytes, the scan's tile sums.
 *
 * atvs_mesh_sample_place.  One lane per sample s in [0, n_samples).  f is the face with offsets[f] <= s < offsets[f + 1] (the last
 * face whose offset is <= s: a face with count 0 is never chosen), j = s - offsets[f], w = hash(k_f, j),
 * u = ((double)(w >> 32) + 0.5) 2^-32, v = ((double)(w & 0xffffffff) + 0.5) 2^-32, and where u + v > 1: u = 1 - u, v = 1 - v (all
 * exact in double).  points (n_samples,3) float32: per axis (a + u e1) + v e2 in double, rounded once.  sample_face (n_samples,)
 * int32: f.  colors_out (n_samples,3) uint8, written when colors is given: per channel rint(((1 - u - v) c_a + u c_b) + v c_c), ties
 * to even, 1 - u - v formed as (1 - u) - v.  normals (n_samples,3) float32, written when the pointer is given: n / sqrt((nx nx + ny
 * ny) + nz nz) in double, rounded once (a face of area 0 has no sample under counts of atvs_mesh_sample_counts).  info: two int64
 * words, zeroed here: [0] = 1 when offsets[n_faces] != n_samples (nothing else is written then), [1] the samples whose face has an
 * index outside 0..n_vertices-1 (sample_face -1, zeros elsewhere; no output is defined unless both words are 0).  A lane's face is
 * always inside 0..n_faces-1 and every store inside the n_samples rows, whatever offsets holds.  n_samples > 0 with n_faces = 0 is
 * ATVS_ERR_SHAPE. */
#define ATVS_MESH_SAMPLE_MAX 268435456
int atvs_mesh_sample_counts(const float* vertices, long n_vertices, const int* faces, long n_faces, double density, long seed,
                            void* counts, double* areas, long* info, atvs_stream_t stream);
int atvs_mesh_sample_scratch_size(long n_faces, long* bytes);
int atvs_mesh_sample_offsets(const void* counts, long n_faces, void* scratch, long scratch_bytes, void* offsets, atvs_stream_t stream);
int atvs_mesh_sample_place(const float* vertices, const void* colors, long n_vertices, const int* faces, long n_faces,
                           const void* offsets, long n_samples, long seed, float* points, int* sample_face, void* colors_out,
                           float* normals, long* info, atvs_stream_t stream);

/* Exact point-to-triangle distances from a cloud to a mesh's surface, so that the half of a score that is measured against a mesh
 * does not depend on a sample spacing: ops/mesh_distance.py, atvsnet/mesh_distance.py, atvsnet/eval_cloud.py --exact_recon /
 * --exact_gt, csrc/mesh_distance.hip; DESIGN.md section 10.3f.  Pointers are device pointers.  tests/mesh_distance_restated.py
 * restates the definition in numpy.  vertices (n_vertices,3) float32, faces (n_faces,3) int32, queries (m,3) float32, radius R > 0
 * (float32).  n_vertices and m in 0..2^30, n_faces in 0..ATVS_MESH_TOPOLOGY_MAX_FACES, max_refs in 0..ATVS_MESH_GRID_MAX_REFS,
 * anything else ATVS_ERR_SHAPE, as is a short grid or scratch; R not a positive finite float32, `cell` not a finite double >= 0, or
 * max_refs < 8 n_faces: ATVS_ERR_ARG; a null pointer that is needed ATVS_ERR_NULL; all without a launch.  No host synchronisation,
 * no allocation.  n_faces = 0, m = 0 and a mesh without a usable face are valid: every query is not found.
 *
 * THE DEFINITION.  A face is USABLE when its three indices are in 0..n_vertices-1 and its nine coordinates are finite.  For a
 * finite query p and a usable face with corners a, b, c (all converted to double; every operation below is a double operation
 * rounded on its own, the library is built with -ffp-contract=off; u.v means (u0 v0 + u1 v1) + u2 v2):
 *     ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c
 *     n  = (ab1 ac2 - ab2 ac1, ab2 ac0 - ab0 ac2, ab0 ac1 - ab1 ac0)
 *     d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp
 *     vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, s = (va + vb) + vc
 * If n is not exactly (0, 0, 0), the closest point x is that of the FIRST region whose test holds:
 *     A         d1 <= 0 and d2 <= 0                         x = a
 *     B         d3 >= 0 and d4 <= d3                        x = b
 *     AB        vc <= 0 and d1 >= 0 and d3 <= 0             t = d1 / (d1 - d3),                     x = a + t ab
 *     C         d6 >= 0 and d5 <= d6                        x = c
 *     AC        vb <= 0 and d2 >= 0 and d6 <= 0             t = d2 / (d2 - d6),                     x = a + t ac
 *     BC        va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0   t = (d4 - d3) / ((d4 - d3) + (d5 - d6)),  x = b + t (c - b)
 *     interior  s > 0                                       v = vb / s, w = vc / s,                 x = (a + v ab) + w ac
 * (the Voronoi-region form of the closest point on a triangle); a quotient whose denominator is not > 0 is taken as 0.  ZERO-AREA
 * FACES.  Where n is exactly (0, 0, 0) -- a repeated vertex makes ab, ac or their difference exactly zero, axis-aligned collinear
 * triples cancel exactly -- and where no test above holds (s <= 0: only roundings on a sliver can do that), the face is the union of
 * its three segments and x comes from the SEGMENT RULE: for (X, Y) = (a, b), (a, c), (b, c) in this order, e = Y - X, w = p - X,
 * t = (w.e) / (e.e) clamped to [0, 1], or 0 where e.e is not > 0 (a point), y = X + t e, and x is the y of the first smallest
 * (p - y).(p - y).  So a face that is a point gives the distance to the point, a collinear triple the distance to the segment it
 * spans, and no quotient is ever 0 / 0.  Every parameter is in [0, 1] (a clamp, or a ratio of a non-negative number to a sum it is
 * part of), so x is a convex combination of the corners whatever the roundings did.  Then r = p - x, d2 = (float)(r.r): rounded ONCE.
 *
 * Per query: d2min = the minimum of d2 over the usable faces, face = the LOWEST face index attaining it -- the 64-bit minimum of
 * (bits(d2) << 32) | face, as atvs_cloud_nearest does for points.  When (double)d2min > (double)R (double)R, or the query is not
 * finite, or no face is usable: d2min = +inf, face = -1.  closest (m,3) float32, written when the pointer is given: (float)x of the
 * attaining face, NaN where face = -1.  The result is a function of the mesh, the queries and R alone: the cell edge, the origin,
 * `cell`, max_refs, the order of the references inside a cell, how many cells hold a face and the launch shape cannot be seen in
 * it.  Integer atomics only.
 *
 * atvs_mesh_grid_build.  grid: atvs_mesh_grid_scratch_size(n_faces, max_refs) bytes; it IS the grid afterwards (a copy of the usable
 * faces' corners included: the search does not read the mesh again).  A uniform grid over the bounding box of the usable faces'
 * corners; cell edge h >= max(R (1 + 2^-18), cell, 2^-60), larger where the box would need more cells than the point-cloud grid's
 * cap for n_faces points; a usable face is referenced from every cell that the box of its corners overlaps (csrc/mesh_distance.hip
 * says why the 27 cells around a query then hold every face within R).  info: four int64 words, [0] the references that h needs,
 * [1] 1 when [0] <= max_refs and the grid was built, else 0: the grid is then NOT searchable (atvs_mesh_nearest reports every
 * query not found) and the caller calls again with a larger `cell`; [2] the usable faces; [3] h as the bits of a double.  Once h
 * reaches the box's extent a face is in at most 8 cells, which is why max_refs >= 8 n_faces is required: a caller that at least
 * doubles `cell` each time ends.
 *
 * atvs_mesh_nearest.  scratch: atvs_mesh_nearest_scratch_size(n_faces, m) bytes (the queries' counting sort by the grid's cells).
 * n_faces and max_refs are those of the build.  d2 (m,) float32, face (m,) int32, closest (m,3) float32 or null: every row is
 * written. */
#define ATVS_MESH_GRID_MAX_REFS 2147483647
int atvs_mesh_grid_scratch_size(long n_faces, long max_refs, long* bytes);
int atvs_mesh_grid_build(const float* vertices, long n_vertices, const int* faces, long n_faces, float radius, double cell,
                         long max_refs, void* grid, long grid_bytes, long* info, atvs_stream_t stream);
int atvs_mesh_nearest_scratch_size(long n_faces, long m, long* bytes);
int atvs_mesh_nearest(const void* grid, long grid_bytes, long n_faces, long max_refs, const float* queries, long m, void* scratch,
                      long scratch_bytes, float* d2, int* face, float* closest, atvs_stream_t stream);

/* A triangle mesh smoothed by Taubin's filter (umbrella weights), and its vertex normals: ops/mesh_smooth.py, atvsnet/smooth_mesh.py,
 * csrc/mesh_smooth.hip; DESIGN.md section 10.3g.  Pointers are device pointers except origin (HOST, 3 finite doubles).  Integer
 * atomics only, no float atomics: every output is a function of the inputs alone, bit for bit on every run -- with ONE exception, the
 * order inside a row of `neighbours` (below), which no result computed from it can show.  No host synchronisation, no allocation;
 * scratch is the caller's.  The library is built with -ffp-contract=off and the definitions rely on it: every operation below is a
 * double operation rounded on its own.  tests/mesh_smooth_restated.py restates the definitions in numpy.  vertices (n_vertices,3)
 * float32, faces (n_faces,3) int32; n_vertices in 0..2^30, n_faces in 0..ATVS_MESH_TOPOLOGY_MAX_FACES, n_neighbours in
 * 0..6 ATVS_MESH_TOPOLOGY_MAX_FACES, anything else ATVS_ERR_SHAPE, as is a short scratch; a bad step, factor, area_unit or origin, or
 * aliased q buffers, ATVS_ERR_ARG; a null pointer that is needed ATVS_ERR_NULL; all without a launch.
 *
 * atvs_mesh_adjacency.  The distinct neighbours of every vertex.  A face is usable when its three indices are in 0..n_vertices-1;
 * the others are counted in info[3] and skipped.  Each usable face gives its three pairs (i0,i1), (i1,i2), (i2,i0), sorted into
 * (lo, hi).  A pair with lo == hi is dropped and counted in info[4]; else a pair that names a vertex with a non-finite coordinate is
 * dropped and counted in info[5] (both per face and pair, not per distinct pair).  The distinct pairs that remain, with the number of
 * faces on each, go into an open-addressing table as atvs_mesh_edge_census does it: 64-bit key (lo << 32) | hi, the smallest power of
 * two of slots that is at least 6 n_faces and at least ATVS_MESH_ADJACENCY_MIN_SLOTS, load at most 0.5, every probe loop bounded by
 * the table.  degree (n_vertices,) int32: the number of distinct neighbours.  flags (n_vertices,) int32: bit 0 = all three
 * coordinates finite; bit 1 = endpoint of a pair with exactly one face (a boundary vertex); bit 2 = endpoint of a pair with more
 * than two faces.  offsets (n_vertices+1,) int32: the exclusive prefix sum of degree, by the point-cloud kernels' scan (6 x 2^28
 * fits).  neighbours (6 n_faces,) int32: the first offsets[n_vertices] entries are written; row v = entries offsets[v] ..
 * offsets[v+1]-1 holds v's distinct neighbours in an ORDER THAT IS NOT DEFINED (it is the order of arrival at a per-vertex cursor).
 * info: seven int64 words, zeroed here: [0] distinct pairs, [1] boundary pairs (one face), [2] non-manifold pairs (more than two
 * faces), [3] faces with an index out of range, [4] self pairs dropped, [5] pairs dropped for a non-finite vertex, [6] pairs that
 * found no slot (impossible at that load).  scratch: atvs_mesh_adjacency_scratch_size(n_vertices, n_faces) bytes: the table (12 bytes
 * a slot), a cursor per vertex and the scan's tile sums.
 *
 * atvs_mesh_quantize.  Positions as integers, so that a sum of neighbours is exact and has no order.  step: a positive power of two.
 * Per coordinate q = llrint(((double)x - origin_a) / step) (ties to even); q (n_vertices,3) int64.  A vertex with a non-finite
 * coordinate gets the row 0, 0, 0.  info: two int64 words, zeroed here: [0] non-finite vertices, [1] coordinates with |q| > 2^31; no
 * output is defined unless [1] is 0.
 *
 * atvs_mesh_smooth_pass.  One umbrella step, one lane per vertex, q_in -> q_out (both (n_vertices,3) int64; they must not alias).
 * factor: a finite double with |factor| <= 1.  A vertex keeps its q_in when it is not finite (flags bit 0 clear), when its degree is
 * 0, or when flags & pin_mask is non-zero.  Otherwise, per axis: S = the exact int64 sum of q_in over the degree[v] entries of
 * neighbours from offsets[v] on; m = (double)S / (double)degree; d = m - (double)q; q_out = q + llrint(factor d), clamped to
 * [-2^32, 2^32].  |q| <= 2^32 and degree < 2^30 keep |S| below 2^62.  info: two int32 words that the CALLER zeroes before its
 * first pass and that every pass adds to (32-bit integer atomics): [0] clamped coordinates (non-zero: the filter has diverged), [1]
 * lanes whose row would leave the n_neighbours entries of `neighbours` or that read an index outside 0..n_vertices-1: they keep
 * q_in.  No load or store leaves its buffer whatever the arrays hold.  No other atomics.
 *
 * atvs_mesh_dequantize.  q, the q0 that atvs_mesh_quantize gave, and its input vertices -> vertices_out (n_vertices,3) float32: a
 * coordinate whose q equals its q0 keeps the BITS of the input coordinate; any other is (float)(origin_a + step (double)q).  So
 * pinned, isolated and non-finite vertices, and zero passes, return the input bits.
 *
 * atvs_mesh_face_extent.  One lane per face: m = (b - a) x (c - a) in double in atvs_mesh_sample_counts' form (differences of
 * (double) coordinates, products then one subtraction per component), s = sqrt((m0 m0 + m1 m1) + m2 m2), twice the area.  info:
 * four int64 words, zeroed here: [0] the maximum of the finite s as the bits of a double (a 64-bit integer atomic max: a non-negative
 * double's bits order as its value), [1] usable faces (indices in range, s finite), [2] faces with an index out of range, [3] faces
 * with a non-finite s.
 *
 * atvs_mesh_vertex_normal_sums.  area_unit: a finite double > 0.  For each face with indices in range and finite s > 0: n = m / s,
 * w = min(1, s / area_unit), and to each of its three vertices llrint((w n_a) 2^30) per axis is added into sums (n_vertices,3) int64
 * with 64-bit integer atomics, and 1 into incidences (n_vertices,) int32; both zeroed here.  A face with a repeated index has m
 * exactly 0 and adds nothing.  At most 3 x 2^28 incidences of terms <= 2^30: no overflow.  With area_unit = the maximum s this is
 * plain area weighting; with a smaller unit every face larger than it votes 1 (atvs_mesh_cluster_quadrics' saturating weight).
 * info: one int32, zeroed here: faces with an index out of range (skipped).
 *
 * atvs_mesh_vertex_normals.  One lane per vertex; the sums are INPUTS.  N = (double)sum, L = sqrt((N0 N0 + N1 N1) + N2 N2); normals
 * (n_vertices,3) float32: (float)(N_a / L) where L > 0, else 0, 0, 0.  Normals point the way the winding says. */
#define ATVS_MESH_ADJACENCY_MIN_SLOTS 1024
int atvs_mesh_adjacency_scratch_size(long n_vertices, long n_faces, long* bytes);
int atvs_mesh_adjacency(const float* vertices, long n_vertices, const int* faces, long n_faces, void* scratch, long scratch_bytes,
                        int* degree, int* flags, int* offsets, int* neighbours, long* info, atvs_stream_t stream);
int atvs_mesh_quantize(const float* vertices, long n_vertices, const double* origin, double step, long* q, long* info,
                       atvs_stream_t stream);
int atvs_mesh_smooth_pass(const long* q_in, long n_vertices, const int* degree, const int* flags, const int* offsets,
                          const int* neighbours, long n_neighbours, double factor, int pin_mask, long* q_out, int* info,
                          atvs_stream_t stream);
int atvs_mesh_dequantize(const long* q, const long* q0, const float* vertices, long n_vertices, const double* origin, double step,
                         float* vertices_out, atvs_stream_t stream);
int atvs_mesh_face_extent(const float* vertices, long n_vertices, const int* faces, long n_faces, long* info, atvs_stream_t stream);
int atvs_mesh_vertex_normal_sums(const float* vertices, long n_vertices, const int* faces, long n_faces, double area_unit, long* sums,
                                 int* incidences, int* info, atvs_stream_t stream);
int atvs_mesh_vertex_normals(const long* sums, long n_vertices, float* normals, atvs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ATVSNET_HIP_H */
