/*
 * frmap_hip.h — C ABI of the MI355X (gfx950) embedding-extraction + gallery-matching kernels.
 *
 * The reference (henryhcooperr/FaceRecognition-MultiArchitecture-Pipeline) has no FFI / plugin
 * boundary of its own: its hot path is stock torch.nn ops called from Python
 * (src/face_models.py, src/app.py).  This header is the boundary a maintainer binds instead; each
 * entry point names the reference lines whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it says "host"; the library never allocates,
 *     frees or synchronises: outputs and scratch are caller-owned, launches are asynchronous on
 *     `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *   - return value: 0 = launched, negative = rejected before any launch (frmap_last_error()
 *     gives the text); nothing is thrown across the ABI;
 *   - `dtype`: FRMAP_BF16 or FRMAP_F16 = storage + MFMA input type of activations / packed conv
 *     weights (accumulation is always fp32); heads and matching are fp32 throughout;
 *   - activations are NHWC ("channels last"), C a multiple of 32 for frmap_conv_igemm;
 *   - pointer alignment: a device pointer must be aligned to the widest access a kernel makes through it.  A call whose pointers
 *     meet the alignment below computes the same bits wherever its buffers start; a pointer below it is rejected (-1, the text
 *     names the entry point, the argument and the bytes) before any launch.  NULL for an optional argument is not checked.
 *     By class of pointer:
 *       tensors in `dtype` (activations, residuals, packed weights, packed galleries, fp16 splits, outputs): 16-byte aligned
 *         (every kernel moves them as 8-element vectors, LDS-DMA fetches included);
 *       fp32 per-channel vectors of the MFMA kernels (`shift` of the convolutions, the stems and frmap_linear_mfma; pos / gamma /
 *         beta of frmap_add_pos_layernorm): 16-byte aligned (read four channels at a time);
 *       fp32 matrices that a GEMM, the exact re-score or the tracker reads in rows of float4 - emb, gallery, a, b, stat_w,
 *         gallery_stat, emb_out of the model calls, x and w of frmap_linear_f32 / frmap_cosine_logits / frmap_arcmargin_eval,
 *         boxes, fused (their row lengths are multiples of 4, or the kernel takes the tail element by element): 16-byte aligned;
 *       everything walked element by element - the fp32 operands and outputs of the other heads (any row length D), per-probe
 *         results (idx_out, dist_out, id_or_unknown_out, packed_out, label_out, count_out ...), int32 / int64 labels, counts and
 *         ids, uint64 counters, uint8 images, the casts: the element size (1, 2, 4 or 8 bytes);
 *       records with 8-byte fields or int32 pairs (frames, items, mats, rows, pair_out): 8-byte aligned;
 *       workspaces and state buffers: 16-byte aligned, 256-byte aligned where the entry point says so.
 *     An argument that departs from its class says so where it is declared.  Where a launcher has a narrower path for some
 *     shapes (odd H * W, D % 512 != 0) it accepts the narrower alignment there; the figure given is the one that always serves.
 *   - threading / devices (the reference calls model(x) from a daemon thread while the main thread
 *     matches, src/app.py:331-335,639): every entry point may be called from any host thread; like
 *     every HIP launch it targets the calling thread's CURRENT device, so the caller makes the
 *     device that owns the pointers and `stream` current first (hipSetDevice; the Python binding
 *     does it per call from the operands' device).  Per-kernel launch attributes are kept per
 *     (kernel, device), so one process may drive several GPUs.
 */
#ifndef FRMAP_HIP_H
#define FRMAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRMAP_BF16 0
#define FRMAP_F16 1

/* Batch-invariant planning.  By default the conv / Linear planners pick a layer's kernel and tile layout from the number of
 * tiles the launch would have (pixel split, in-workgroup split-K, first- or second-generation kernel), i.e. from the batch size:
 * the same face then gets different fp32 summation orders - results equal to rounding, not to the bit - in batches of
 * different sizes.  on = 1: layouts are chosen from the per-image geometry alone (never split-K by tile count), so a face's
 * embedding and match are bit-identical whatever batch, shard or rank it is computed in, at some cost in speed for small
 * batches.  on = 0: default planning; on = -1: back to the environment (FRMAP_BATCH_INVARIANT=1).  Process-wide. */
int frmap_set_batch_invariant(int on);

/* ABI version of this header (bumped on any signature change). */
int frmap_abi_version(void);
/* Text of the last rejected call on this thread ("" if none). Host pointer, do not free. */
const char* frmap_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Input layout: fp32 NCHW B×3×H×W  ->  NHWC4 (3 channels + one zero channel) in `dtype`.
 * Replaces the implicit layout the reference feeds nn.Conv2d with (src/testing.py:99-104,251).
 * x_nchw needs its element size and out_nhwc4 is 8-byte aligned (one pixel per store): with an even H * W, x_nchw 8-byte and
 * out_nhwc4 16-byte aligned the launcher takes the path that moves two pixels at a time, otherwise the one-pixel path.  Same bits.
 * ------------------------------------------------------------------------------------------- */
int frmap_pack_input_nchw_f32(const float* x_nchw, void* out_nhwc4, int B, int H, int W,
                              int dtype, void* stream);

/* uint8 HWC RGB B×H×W×3 -> ToTensor (u/255) + Normalize ((x-mean)/std), src/testing.py:99-104,
 * src/app.py:39-42.  Writes fp32 NCHW (out_nchw_f32) and/or NHWC4 `dtype` (out_nhwc4); either may be
 * NULL.  mean3_host / std3_host: 3 floats each in HOST memory.  out_nhwc4: 8-byte aligned (one pixel = 8 bytes per store). */
int frmap_normalize_u8_hwc(const unsigned char* img_u8, float* out_nchw_f32, void* out_nhwc4, int B, int H,
                           int W, const float* mean3_host, const float* std3_host, int dtype, void* stream);

/* `transforms.Resize((H, W))` for PIL-style 8-bit RGB images (src/testing.py:99-100, 561-566; src/training.py:305-310;
 * src/app.py:39), batched, bit-exact with Pillow's two-pass bilinear resampler (libImaging/Resample.c: integer FIR taps
 * with 22 fractional bits, the horizontal pass rounded to 8 bits before the vertical pass).  src_pool: the images' bytes
 * (HWC uint8 RGB, native sizes) back to back; items: B records
 *     struct { uint64 src_off; int32 H, W, bx_off, kx_off, ksx, by_off, ky_off, ksy; }      (40 bytes, device memory)
 * with offsets (int32 elements) into `tables` of the per-axis bounds [out][2] = (first input sample, taps) and coefficients
 * [out][ks] (ks = 0: that axis keeps its size) - built by the host in float64 with Pillow's operation order
 * (resize.py:bilinear_coeffs).  out: B x out_h x out_w x 3 uint8.  One workgroup resizes rows_per_block output rows;
 * lds_rows = the most input rows one workgroup touches (lds_rows * out_w * 4 bytes of LDS).  src_pool and out are byte-addressed. */
int frmap_resize_bilinear_u8(const unsigned char* src_pool, const void* items, const int* tables, unsigned char* out,
                             int B, int out_h, int out_w, int rows_per_block, int lds_rows, void* stream);

/* Face crops from device-resident frames in one launch: `frame[y1:y2, x1:x2]` (src/app.py:234), the BGR -> RGB flip and
 * `transforms.Resize` of get_embedding (src/app.py:32-39), for every box of a detector at once.  Output i is bit-identical to
 * PIL.Image.fromarray(rgb_frame[y1:y2, x1:x2]).resize((out_w, out_h), BILINEAR): the integer arithmetic of
 * frmap_resize_bilinear_u8, with the filter taps computed ON THE DEVICE (Pillow's precompute_coeffs + normalize_coeffs_8bpc in
 * float64, Pillow's operation order, nothing fused) - no host tables, no host work per box size, nothing synchronised.
 *   frames : n_frames records  struct { uint64 base; int32 H, W; int64 pitch; }   (24 bytes, device memory)
 *            base = device address of pixel (0, 0) of an HWC uint8 frame, pitch = bytes per row (>= 3 * W)
 *   rois   : N records  int32 { frame, x1, y1, x2, y2 }   (20 bytes, device memory): rows [y1, y2), columns [x1, x2) of that
 *            frame, 0 <= x1 < x2 <= W, 0 <= y1 < y2 <= H.  Device data: NOT validated by this call (the Python wrapper does it
 *            before the upload); the kernel skips a record that breaks the contract or exceeds max_roi_* and leaves its output
 *            unwritten, so nothing is read outside a frame.
 *   bgr    : != 0: the frames are BGR (cv2), swapped to RGB on read
 *   out    : N x out_h x out_w x 3 uint8 RGB
 *   max_roi_h, max_roi_w : host-side upper bounds of the ROI sizes (the frame size always serves); they size the launch: one
 *            workgroup resizes up to 8 output rows, fewer when the input rows those touch would not fit LDS.
 * Supported reduction: the LDS need (4 * out_w * (5 c + 5) bytes for a c-fold reduction at one row per workgroup) must fit
 * 160 KB - every ROI that shrinks by at most 32x per axis to an output at most 224 wide does; beyond that the call is rejected.
 * Not covered: Pillow resizes an image more than 100x taller than wide whose height shrinks in the other order (height first);
 * the Python wrapper routes such ROIs through frmap_resize_bilinear_u8.  N < 0, null pointers and bad shapes are rejected before
 * any launch; N == 0 returns 0 and launches nothing. */
int frmap_crop_resize_u8(const void* frames, int n_frames, const int32_t* rois, unsigned char* out, int N, int out_h,
                         int out_w, int max_roi_h, int max_roi_w, int bgr, void* stream);
/* The filter taps the crop kernel computes, from the same function compiled for the CPU (HOST pointers; no GPU needed):
 * ksize_out = taps per output sample (ceil(max(in / out, 1)) * 2 + 1); bounds_out int32 [out_size][2] = (first input sample,
 * taps); coeffs_out int32 [out_size][ksize], zero past a sample's taps.  bounds_out and coeffs_out may both be NULL (ksize only). */
int frmap_resize_coeffs_host(int in_size, int out_size, int32_t* bounds_out, int32_t* coeffs_out, int* ksize_out);

/* Eye-aligned face crops in one launch: frmap_crop_resize_u8 on the frame ROTATED about a point (the reference's dataset step,
 * src/data_prep.py:69-87, 144-150: rotate the whole image until the eye line is level, crop the box, resize), without a rotated
 * frame ever written to memory.  The geometry is the reference's; the RESAMPLING IS PILLOW'S, NOT cv2's (the reference calls
 * cv2.warpAffine / cv2.resize, which sample another grid with fixed-point weights): output i is bit-identical to
 *   PIL.Image.fromarray(rgb_frame).rotate(angle, resample=BILINEAR, center=c).crop((x1, y1, x2, y2)).resize((out_w, out_h), BILINEAR)
 *   frames, rois, out, bgr, max_roi_h, max_roi_w : as frmap_crop_resize_u8; the ROI is in the rotated frame's coordinates (the
 *            rotated frame has the frame's size; what rotates in from outside is 0)
 *   mats   : N x 6 float64 (device memory, 8-byte aligned): Image.rotate's output -> input matrix (a, b, c, d, e, f) of each face,
 *            computed by the host (Pillow rounds cos / sin to 15 decimals; frames.rotation_matrix in the Python package).  Source
 *            position of output pixel (x, y): (a (x + 0.5) + b (y + 0.5) + c, d (x + 0.5) + e (y + 0.5) + f), float64, unfused.
 * With out_h x out_w equal to the ROI's size the output is the rotated crop itself.  Device records are NOT validated by this call:
 * the kernel skips a record whose ROI or frame index breaks the contract, whose matrix holds a non-finite entry or whose window
 * exceeds max_roi_*, and leaves its output unwritten; every source index is clamped, so nothing is read outside a frame.  Supported
 * reductions, the tall-ROI exception and the host-side rejections are those of frmap_crop_resize_u8. */
int frmap_align_crop_resize_u8(const void* frames, int n_frames, const int32_t* rois, const double* mats, unsigned char* out, int N,
                               int out_h, int out_w, int max_roi_h, int max_roi_w, int bgr, void* stream);
/* The rotated crop the kernel resizes, from the same function compiled for the CPU (HOST pointers; no GPU needed): rows [y1, y2),
 * columns [x1, x2) of Image.rotate's output for the H x W frame (3 bytes per pixel, `pitch` bytes per row) and the matrix mat6,
 * written as [y2 - y1][x2 - x1][3] RGB (bgr != 0: the frame is BGR).  Null pointers, a ROI that is empty or leaves the frame and a
 * non-finite matrix are rejected. */
int frmap_align_warp_host(const unsigned char* frame, int H, int W, long long pitch, const double* mat6, int x1, int y1, int x2,
                          int y2, int bgr, unsigned char* out);

/* Face crops straight from 4:2:0 YUV frames with 8-bit samples (NV12 / NV21 decoder surfaces, planar I420 / YV12) in one launch:
 * output i is bit-identical to frmap_crop_resize_u8 on the frame CONVERTED to RGB by this rule, and no RGB frame is written:
 *   chroma : pixel (x, y) takes chroma sample (x >> 1, y >> 1) - nearest replication; the chroma planes are ceil(H/2) x ceil(W/2)
 *   colour : int32, arithmetic shift, clip8 = clamp to [0, 255], the pixel rounded to uint8 RGB before any filter tap reads it
 *              R = clip8((cy (Y - y_off) + rv (V - 128) + 32768) >> 16)
 *              G = clip8((cy (Y - y_off) + gu (U - 128) + gv (V - 128) + 32768) >> 16)
 *              B = clip8((cy (Y - y_off) + bu (U - 128) + 32768) >> 16)
 *            csc  standard, range    y_off     cy      rv      gu      gv      bu      (each floor(c * 65536 + 0.5) of its float64
 *             0   bt601, limited       16   76309  104597  -25675  -53279  132201       value from (Kr, Kb) and the range scaling;
 *             1   bt601, full           0   65536   91881  -22553  -46802  116130       at most 1 away from the rounded float64
 *             2   bt709, limited       16   76309  117489  -13975  -34925  138438       formula, for every (Y, U, V))
 *             3   bt709, full           0   65536  103206  -12276  -30679  121609
 *   frames : n_frames records of 56 bytes in device memory, in this order: uint64 y, u, v (device addresses of sample (0, 0) of
 *            the luma and the two chroma planes); int32 H, W; int64 y_pitch, c_pitch (bytes per row of the luma plane and of a
 *            chroma plane: >= W, >= c_step * ceil(W/2)); int32 c_step (bytes from one chroma sample to the next in its row: 1 =
 *            planar, 2 = interleaved); int32 csc (the table's row).  NV12: v = u + 1, c_step = 2.  NV21: u = v + 1, c_step = 2.
 *            I420 / YV12: three planes, c_step = 1.  Frames of one call may differ in size, layout and csc.  Odd H and W are allowed.
 *   rois, out, max_roi_h, max_roi_w : as frmap_crop_resize_u8 (there is no bgr flag: the output is RGB).
 * Device records are NOT validated by this call: the kernel skips a record - its output stays unwritten, nothing is read or
 * written outside the buffers - whose frame index is out of range, whose ROI is empty or leaves the frame, whose frame has a null
 * plane, c_step outside {1, 2}, csc outside [0, 4), y_pitch < W or c_pitch < c_step * ceil(W/2), or whose window exceeds
 * max_roi_*.  Supported reductions, the tall-ROI exception and the host-side rejections are those of frmap_crop_resize_u8. */
int frmap_crop_resize_yuv(const void* frames, int n_frames, const int32_t* rois, unsigned char* out, int N, int out_h, int out_w,
                          int max_roi_h, int max_roi_w, void* stream);
/* frmap_align_crop_resize_u8 on YUV frames: bit-identical to it on the converted frame.  The four corner pixels of each bilinear
 * warp sample are converted to uint8 RGB first, Pillow's float64 warp then runs on those; a sample outside the frame is RGB
 * (0, 0, 0).  frames: the 56-byte records above; mats: as frmap_align_crop_resize_u8 (a non-finite entry: the record is skipped). */
int frmap_align_crop_resize_yuv(const void* frames, int n_frames, const int32_t* rois, const double* mats, unsigned char* out, int N,
                                int out_h, int out_w, int max_roi_h, int max_roi_w, void* stream);
/* The conversion the YUV kernels apply per pixel, from the same function compiled for the CPU (HOST pointers; no GPU needed):
 * the whole H x W frame as out_rgb [H][W][3].  Null pointers, H or W < 1, c_step outside {1, 2}, csc outside [0, 4) and a pitch
 * below its row are rejected before anything is written. */
int frmap_yuv_to_rgb_host(const unsigned char* y, const unsigned char* u, const unsigned char* v, int H, int W, long long y_pitch,
                          long long c_pitch, int c_step, int csc, unsigned char* out_rgb);
/* frmap_align_warp_host for a YUV frame: rows [y1, y2), columns [x1, x2) of Image.rotate's output for the converted frame, written
 * as [y2 - y1][x2 - x1][3] RGB.  Rejections: those of frmap_yuv_to_rgb_host and of frmap_align_warp_host. */
int frmap_yuv_align_warp_host(const unsigned char* y, const unsigned char* u, const unsigned char* v, int H, int W, long long y_pitch,
                              long long c_pitch, int c_step, int csc, const double* mat6, int x1, int y1, int x2, int y2,
                              unsigned char* out);

/* The frame loop's IoU tracker (src/app.py:126-147, 183-247: process_webcam's face_id that survives from frame to frame), one
 * launch for n_streams independent streams (cameras, or clips stepped together), the per-stream state resident on the device.
 * One step of one stream, given its n = counts[s] detections in the detector's order and its frame's size (H, W):
 *   - n == 0: the state is left exactly as it is (tracks survive a frame without detections);
 *   - detection i is SKIPPED (id -1) when probs[i] < det_thresh compared in float32 (a probability equal to (float)det_thresh is
 *     kept), when a coordinate or the probability is not finite, or when its integer crop - truncate toward zero, max(0, .),
 *     min(W or H, .): frames.clip_boxes' rule - has x2 <= x1 or y2 <= y1;
 *   - otherwise the previous boxes j = 0 .. P - 1 not yet matched in this step are scanned in ascending order and j replaces the
 *     best so far when iou(box_i, prev_j) > best (which starts at 0) and > iou_thresh: ties go to the lowest j.  A winner gives
 *     its id and becomes matched; without one the detection takes id = next_id, and next_id grows by one;
 *   - the new state is the raw boxes and ids of the detections that received an id, in order (none: empty); next_id is never
 *     reset (ids stay below 2^31 per stream).
 * iou is calc_iou's operation order on the RAW boxes.  DEPARTURES from the reference: (a) the IoU arithmetic is float64 on the
 * float32 inputs with nothing fused - the reference mixes np.float32 rows with Python floats, so the precision of each of its
 * operations depends on which operand a max() returned and on the NumPy version; the two can differ only where an IoU lies within
 * float32 rounding of the threshold or of a competing IoU; (b) the state keeps only boxes that received an id - the reference
 * rebuilds its box list from every confident box and its id list from the boxes with an id, so a confident box with an empty crop
 * puts its two lists out of step.
 *
 * State buffer (frmap_track_state_bytes(n_streams, max_boxes) bytes, 16-byte aligned, caller-owned; 0 for unsupported sizes):
 * int32 meta[n_streams][2] = (P, next_id) at byte 0; float32 boxes[n_streams][max_boxes][4] at the next multiple of 16 bytes
 * after the meta records; int32 ids[n_streams][max_boxes] right after the boxes.  All-zero bytes are a fresh state (P = 0,
 * next_id = 0); zeroing one stream's meta record resets that stream.
 *   boxes    : float32 [n_streams][max_boxes][4] = (x1, y1, x2, y2) as the detector returns them, 16-byte aligned
 *   probs    : float32 [n_streams][max_boxes], or NULL: every box is confident (as clip_boxes' probs = None)
 *   counts   : int32 [n_streams]; frame_hw : int32 [n_streams][2] = (H, W)
 *   ids_out  : int32 [n_streams][max_boxes]: the id, -1 for skipped detections and for slots beyond counts[s]
 *   rois_out : int32 [n_streams][max_boxes][4], 16-byte aligned: the integer crop (x1, y1, x2, y2) of every detection that got an id,
 *              0 in every other slot
 * Supported: 1 <= max_boxes <= 256; anything else, n_streams < 0 and null or misaligned pointers are rejected before any launch,
 * nothing is ever truncated.  counts is DEVICE data this call never sees: the kernel clamps it to [0, max_boxes] (and the state's
 * P likewise) and never reads or writes outside its stream's slots; a caller that builds counts on the host rejects
 * counts[s] > max_boxes there (the Python package does).  One wavefront per stream; no atomics. */
size_t frmap_track_state_bytes(int n_streams, int max_boxes);
int frmap_track_step(void* state, const float* boxes, const float* probs, const int32_t* counts, const int32_t* frame_hw,
                     int n_streams, int max_boxes, double det_thresh, double iou_thresh, int32_t* ids_out, int32_t* rois_out,
                     void* stream);
/* The same step from the same rule compiled for the CPU (HOST pointers, no stream; no GPU needed).  counts[s] outside
 * [0, max_boxes] is rejected, like every other bad argument, before anything is written. */
int frmap_track_step_host(void* state, const float* boxes, const float* probs, const int32_t* counts, const int32_t* frame_hw,
                          int n_streams, int max_boxes, double det_thresh, double iou_thresh, int32_t* ids_out, int32_t* rois_out);

/* Track templates: the embeddings of a track (a face_id of frmap_track_step) pooled on the device, one launch per step for
 * n_streams streams between the model and the match.  Per stream the state is a list of slots (id, weight w, sum[dim]); one step
 * of one stream, given the tracker's ids of this step (ids[s][0 .. counts[s]), -1 = skipped), the step's embedding rows emb
 * [n_rows][dim] and rows [n_rows][2] = (stream, detection index) of each row:
 *   - counts[s] == 0: the state is left exactly as it is;
 *   - otherwise the new state has one slot per detection with id >= 0, in detection order (the tracker's own state after that
 *     step, slot for slot); old ids that are absent are dropped;
 *   - a detection whose id is in the old state and that has a row of finite values: w' = fl(fl(decay w) + 1), sum'[d] =
 *     fl(fl(decay sum[d]) + e[d]) - float32, two roundings, nothing fused; an id that is new: w' = 1, sum' = e;
 *   - without a row, or with a row that holds an infinity or a NaN, the old slot is carried over unchanged (a new id: w' = 0,
 *     sum' = 0);
 *   - fused[r] = sum' / w' (correctly rounded) and frames_out[r] = w' for the row of such a detection; a row whose detection has
 *     id < 0, that is not finite or whose slot has w' == 0 is copied to fused[r] bit for bit, with frames_out[r] = 0.
 * State buffer (frmap_track_fuse_state_bytes(n_streams, max_boxes, dim) bytes, 16-byte aligned, caller-owned; 0 for unsupported
 * sizes): int32 meta[n_streams][2] = (P, current bank) at byte 0; then, from the next multiple of 16 bytes, int32
 * ids[n_streams][2][max_boxes], float32 w[n_streams][2][max_boxes] and float32 sum[n_streams][2][max_boxes][dim rounded up to 4]:
 * two banks of slots per stream - a step reads the current one and writes the other, because a track's slot moves with the
 * detector's order.  All-zero bytes are a fresh state; zeroing one stream's meta record resets that stream.
 *   ids, counts : the tracker's int32 [n_streams][max_boxes] and [n_streams] of this step
 *   emb, fused  : float32 [n_rows][dim], 16-byte aligned, distinct; frames_out: float32 [n_rows]; rows: int32, 8-byte aligned
 *   decay       : 0 < decay <= 1 (1: the plain mean of the track's embeddings)
 * Supported: 1 <= max_boxes <= 256, 1 <= dim <= 4096, n_rows <= n_streams * max_boxes; anything else is rejected before any
 * launch.  counts, ids and rows are DEVICE data this call never sees: the kernel clamps counts (and the state's P), lets a row take
 * part only if it names a detection of its stream below that count, and never touches another stream's slots; a row that names no
 * detection is passed through, and of two rows that name the same detection one (either) is pooled and the other passed through - a
 * caller that builds rows on the host rejects both there (the Python package does).  One workgroup per stream; no atomics. */
size_t frmap_track_fuse_state_bytes(int n_streams, int max_boxes, int dim);
int frmap_track_fuse(void* state, const int32_t* ids, const int32_t* counts, const float* emb, const int32_t* rows, int n_rows,
                     int n_streams, int max_boxes, int dim, float decay, float* fused, float* frames_out, void* stream);
/* The same step from the same rule compiled for the CPU (HOST pointers, no stream; no GPU needed).  A count outside
 * [0, max_boxes], a row that names a stream outside [0, n_streams) or a detection outside [0, counts[stream]) and two rows that
 * name the same detection are rejected, like every other bad argument, before anything is written. */
int frmap_track_fuse_host(void* state, const int32_t* ids, const int32_t* counts, const float* emb, const int32_t* rows, int n_rows,
                          int n_streams, int max_boxes, int dim, float decay, float* fused, float* frames_out);

/* ---------------------------------------------------------------------------------------------
 * Conv weight packing.  `w_oihw` = fp32 [Cout][Cin][KH][KW] with the BatchNorm scale already
 * folded in (w * gamma/sqrt(var+eps)); output is the kernel's LDS-image order in `dtype`.
 *   frmap_pack_conv_weight      : for frmap_conv_igemm      (Cin % 32 == 0, Cout % 64 == 0,
 *                                 KH == KW in {1,3});  out elems = Cout*Cin*KH*KW
 *   frmap_pack_conv_weight_c3   : for frmap_conv_small_cin  (Cin == 3);  out elems =
 *                                 Cout * frmap_small_cin_kpad(KH, KW)
 * The packers write w_packed element by element: 2-byte aligned serves here; the convolutions that read it need 16.
 * ------------------------------------------------------------------------------------------- */
int frmap_pack_conv_weight(const float* w_oihw, void* w_packed, int Cout, int Cin, int KH, int KW,
                           int dtype, void* stream);
int frmap_small_cin_kpad(int KH, int KW);
int frmap_pack_conv_weight_c3(const float* w_oihw, void* w_packed, int Cout, int KH, int KW,
                              int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * First-layer convolution on NHWC4 input (Cin = 3) + per-channel shift + optional ReLU.
 *   ResNet/Siamese stem 7x7 s2 p3 -> 64   (torchvision resnet18.conv1/bn1/relu via
 *                                          src/face_models.py:67,463,658; face_models.py:115-117)
 *   BaselineNet conv1 3x3 s1 p1 -> 32     (src/face_models.py:21-22,38)
 * Implicit GEMM on v_mfma_f32_16x16x32 with the K axis laid along (kw, c) of each kernel row.
 * out: NHWC B×Ho×Wo×Cout in `dtype`.  Cout in {32, 64}.  in_nhwc4: 8-byte aligned (pixels are staged one 8-byte pixel at a time).
 * Non-finite input ("Non-finite values"): a NaN / inf pixel makes every output of its receptive field NaN / inf as
 * in PyTorch (the ReLU keeps NaN) and may also make NaN the outputs whose zero-weight pad taps read it (same image, one pixel
 * column beside the field; 3x3: the output row below as well); no other output and no other image changes by a bit.
 * ------------------------------------------------------------------------------------------- */
int frmap_conv_small_cin(const void* in_nhwc4, const void* w_packed, const float* shift, void* out,
                         int B, int Hi, int Wi, int Cout, int KH, int KW, int stride, int pad,
                         int relu, int dtype, void* stream);
/* The 3x3 s1 p1 3->32 layer with MaxPool2d(2, 2) fused into its epilogue: BaselineNet
 * `self.pool(F.relu(self.bn1(self.conv1(x))))` (src/face_models.py:38) in one launch.  The kernel walks
 * its output pixels in pool-major order (4 consecutive pixels = one 2x2 window), so the pooled value is
 * a max over 4 accumulator rows; the 32×H×W conv map never reaches HBM.  Even Hi, Wi.
 * out: B×(Hi/2)×(Wi/2)×32.  Non-finite values: as frmap_conv_small_cin followed by frmap_maxpool, bit for bit.
 * in_nhwc4: 8-byte aligned, as frmap_conv_small_cin. */
int frmap_conv_small_cin_pool2(const void* in_nhwc4, const void* w_packed, const float* shift, void* out,
                               int B, int Hi, int Wi, int Cout, int relu, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused ResNet stem: fp32 NCHW B×3×Hi×Wi -> conv 7x7 s2 p3 (3->64) + shift + ReLU -> maxpool 3x3 s2 p1
 * -> NHWC B×Hq×Wq×64 in `dtype`, one kernel (the 64×112×112 conv map never reaches HBM).
 * Replaces conv1/bn1/relu/maxpool of torchvision resnet18 (src/face_models.py:67,463,658) plus the
 * input layout cast.  w_packed_c3: from frmap_pack_conv_weight_c3(…, 64, 7, 7).  Needs Wi <= ~224
 * (pooled width <= 56); wider inputs use frmap_pack_input + frmap_conv_small_cin + frmap_maxpool.
 * x_nchw needs its element size only (4 bytes): a 16-byte aligned tensor with Wi % 4 == 0 is staged with 16-byte loads (and takes
 * the second-generation kernel), any other through the scalar staging path of the first-generation kernel.  frmap_stem7x7_maxpool2
 * gives the same bits either way; frmap_stem7x7_maxpool sums a pixel's products in another order in its two kernels, so the same
 * image at a 4-byte and at a 16-byte aligned address may differ in the last place of a few outputs (both within one rounding).
 * Non-finite input (all four stem entry points): a NaN / inf pixel, or an fp32 pixel beyond the range of `dtype`, reaches every
 * pooled output whose window holds a conv position of its receptive field, as nn.ReLU + nn.MaxPool2d propagate it (a window
 * keeps a NaN, drops a -inf), and may make NaN the windows holding a conv position whose zero-weight pad tap reads it (one pixel
 * column / row beside the field, same image).  Nothing else changes by a bit; a NaN / inf `shift` reaches its channel.
 * ------------------------------------------------------------------------------------------- */
int frmap_stem7x7_maxpool(const float* x_nchw, const void* w_packed_c3, const float* shift, void* out,
                          int B, int Hi, int Wi, int dtype, void* stream);
/* Same fusion with MaxPool2d(2, 2): SiameseNet conv.0-3 (conv 7x7 s2 p3 + bias + BN + ReLU + pool,
 * src/face_models.py:115-118); out = B×(Hc/2)×(Wc/2)×64. */
int frmap_stem7x7_maxpool2(const float* x_nchw, const void* w_packed_c3, const float* shift, void* out,
                           int B, int Hi, int Wi, int dtype, void* stream);
/* The same two fusions fed by the uint8 image itself: x_u8_hwc = B×Hi×Wi×3 RGB bytes (what
 * transforms.Resize leaves, src/testing.py:99-100); ToTensor (u/255) + Normalize((x-mean)/std)
 * (src/testing.py:101-104; mean/std: 3 floats each in HOST memory) are applied while the rows are
 * staged, through a per-channel 256-entry table rounded to `dtype` exactly as
 * frmap_normalize_u8_hwc + the fp32 entry points would — the 602 KB/face fp32 tensor never exists
 * (SURVEY.md §8f row 1).  pool3 != 0: MaxPool2d(3,2,1) (ResNet stem); 0: MaxPool2d(2,2) (Siamese).
 * Needs Wi % 4 == 0 and x_u8_hwc 4-byte aligned (4 pixels = 12 bytes are read as three dwords). */
int frmap_stem7x7_maxpool_u8(const unsigned char* x_u8_hwc, const float* mean3_host, const float* std3_host,
                             const void* w_packed_c3, const float* shift, void* out, int B, int Hi, int Wi,
                             int pool3, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution, NHWC, MFMA 16x16x32 (bf16 / f16), fused epilogue
 *     out = act( conv(in, w) + shift[cout] [+ residual] )      act (`relu` argument): 0 none, 1 ReLU,
 *                                                              2 exact GELU (nn.GELU, face_models.py:630)
 * Covers: every 3x3 (s1/s2, p1) and 1x1 (s1/s2, p0) convolution + folded BatchNorm (+ReLU)
 * (+ residual add) of the ResNet-18 BasicBlocks behind src/face_models.py:67,463,658, of
 * BaselineNet conv2/conv3 (src/face_models.py:23-26,39-40), of SiameseNet (src/face_models.py:
 * 121-141), and — as a 1x1 "conv" over H=W=1 — the wide Linear(+BatchNorm1d)(+ReLU) layers
 * (src/face_models.py:148-155, 629-632).
 *   in       : B×Hi×Wi×Cin   (dtype)
 *   w_packed : from frmap_pack_conv_weight
 *   shift    : fp32 [Cout]   (beta - mean*scale [+ bias*scale])
 *   residual : B×Ho×Wo×Cout (dtype) or NULL
 *   out      : B×Ho×Wo×Cout (dtype),  Ho = (Hi + 2*pad - K)/stride + 1
 * Non-finite values (this entry point, _pool2, _ds and frmap_linear_mfma): a NaN / inf element of `in`, `residual` or `ds_in`
 * gives every output of its receptive field the class (NaN, +inf, -inf, finite) of the same op in PyTorch - ReLU keeps NaN and
 * maps -inf to exactly 0, a value beyond the range of `dtype` is stored as inf - and changes no other output, and no other
 * image, by a bit.
 * ------------------------------------------------------------------------------------------- */
int frmap_conv_igemm(const void* in, const void* w_packed, const float* shift, const void* residual,
                     void* out, int B, int Hi, int Wi, int Cin, int Cout, int K, int stride, int pad,
                     int relu, int dtype, void* stream);
/* conv 3x3 s1 p1 + shift (+ReLU) + MaxPool2d(2, 2) in one launch: BaselineNet conv2/conv3 blocks
 * (src/face_models.py:39-40) and SiameseNet's conv -> BN -> ReLU -> MaxPool2d(2) runs (:121-141).
 * relu in {0, 1} (the max is taken before shift + activation, which is exact for monotonic ones; it keeps a NaN and drops a
 * -inf like nn.MaxPool2d, so the result holds the bits of frmap_conv_igemm + frmap_maxpool for non-finite operands too).
 * out: B×(Hi/2)×(Wi/2)×Cout.  frmap_conv_igemm_pool2_supported: 1 when the shape is taken (even Hi and Wi,
 * Cin % 32 == 0, Cout % 64 == 0, the tile's input rows fit LDS); otherwise run frmap_conv_igemm +
 * frmap_maxpool. */
int frmap_conv_igemm_pool2_supported(int B, int Hi, int Wi, int Cin, int Cout);
/* which kernel frmap_conv_igemm_pool2 runs the shape on: 3 = LDS-DMA ping-pong kernel (row pairs tile a 112-pixel
 * slice: Wi in {2,4,8,14,28,56}, Cin >= 128, Cout % 128 == 0), 2 = weights-resident wave kernel (Cin 32 / 64, Hi and Wi
 * multiples of 8), 1 = generic kernel, 0 = not taken.  frmap_conv3x3_pp_pool_layout: 1 when the ping-pong form fits. */
int frmap_conv_igemm_pool2_form(int B, int Hi, int Wi, int Cin, int Cout);
/* does a 1x1 conv / Linear layer (stride s, pad 0; Linear: Hi = Wi = 1, B = rows) take the LDS-DMA ping-pong kernel
 * (conv1x1_pp_kernel)?  1 = 224 px x 256 ch tiles, 2 = 448 px x 128 ch, 3 = 224 px x 128 ch with split-K, 0 = the
 * first-generation 1x1 kernel runs it (Cin % 32, Cout % 128, too few tiles). */
int frmap_conv1x1_pp_layout(int B, int Hi, int Wi, int Cin, int Cout, int stride);
int frmap_conv3x3_pp_pool_layout(int B, int Hi, int Wi, int Cin, int Cout);
int frmap_conv_igemm_pool2(const void* in, const void* w_packed, const float* shift, void* out, int B, int Hi,
                           int Wi, int Cin, int Cout, int relu, int dtype, void* stream);

/* Tuning / test hook for the second-generation 3x3 stride-1 kernel behind frmap_conv_igemm (conv_pp.hip: 8-wave
 * workgroups, LDS-DMA operands): enable (0 / 1, -1 = default), pixels per tile (<= 224, -1 = whole rows / images),
 * channel tile (128 / 256; 1282 = 128 channels with the wave groups splitting K; -1 = heuristic).  Process-wide; not
 * needed for normal use. */
int frmap_conv_pp_tuning(int enable, int tile_px, int bn);
/* A/B hook of the second-generation kernel's fragment-read placement: 1 = reads of k-step k + 1 interleaved with the
 * MFMAs of k-step k (conv3x3_pp_kernel<..., RI = true>) where the layout allows, 0 = one burst per phase, -1 = environment
 * (FRMAP_PP_RI). */
int frmap_conv_pp_ri(int v);
/* Further process-wide A/B hooks of the same kernel family (experiments recorded in DESIGN.md; defaults = the shipped path):
 * frmap_conv_pp_pitch: conflict-free LDS halo pitch on (1) / off (0); frmap_conv_pp_ds: the fused projection-shortcut form
 * on the second-generation kernel on (1) / off (0); frmap_conv_pp_im: LDS-DMA issued between the MFMAs (1) or in a burst (0). */
int frmap_conv_pp_pitch(int v);
int frmap_conv_pp_ds(int v);
int frmap_conv_pp_im(int v);
/* A/B and test hook of the layer-1 kernel's start-up (conv3x3_c64_wave_kernel, with or without the fused pool): 1 = the first
 * tile's halo loads and every piece of the resident weight slab are issued at once, 0 = the slab piece by piece, then the halo
 * (the form before), -1 = environment (FRMAP_WAVE_START, default 1).  The tile loop is the same: outputs are bit-identical. */
int frmap_conv_wave_start(int v);
/* Which layout frmap_conv_igemm gives a 3x3 stride-1 pad-1 layer without a fused shortcut: 0 = a first-generation
 * kernel; conv3x3_pp_kernel with 1 = 224 px x 256 ch tiles, 2 = 448 px x 128 ch, 3 = 224 px x 128 ch split-K. */
int frmap_conv3x3_pp_layout(int B, int Hi, int Wi, int Cin, int Cout);
/* The same question for a 3x3 stride-2 pad-1 layer (conv3x3s2_pp_kernel: 1 = 224 px x 256 ch, 2 = 448 px x 128 ch). */
int frmap_conv3x3s2_pp_layout(int B, int Hi, int Wi, int Cin, int Cout);
/* ... and for frmap_conv_igemm_ds (3x3 stride-1 layer with a fused 1x1 stride-s projection shortcut): 0 / 1 / 2. */
int frmap_conv3x3_pp_ds_layout(int B, int Hi, int Wi, int Cin, int Cout, int ds_Hi, int ds_Wi, int ds_Cin, int ds_stride);
/* Output pixels per tile of the launch frmap_conv_igemm (ds_Cin == 0; stride 1 or 2) or frmap_conv_igemm_ds (ds_Cin > 0) makes
 * for a 3x3 pad-1 layer on a second-generation kernel; 0 = another kernel runs it.  The layouts above say how many pixels a
 * tile can hold; the launch fills it with whole rows as far as the halo allows (FRMAP_PP_FILL=0, or a tile size forced through
 * frmap_conv_pp_tuning: whole images, or a divisor of the image height). */
int frmap_conv3x3_pp_tile_px(int B, int Hi, int Wi, int Cin, int Cout, int stride, int ds_Hi, int ds_Wi, int ds_Cin, int ds_stride);
/* Which kernel instantiation runs a layer.  Every instantiation the conv launchers can dispatch has one canonical name (its
 * key): the kernel and the template arguments its plan decides, without the data type, e.g. "conv_igemm_kernel<128,3,2>",
 * "conv3x3_pp_kernel<7,2,5,1,DS>", "conv3x3_c64_wave_kernel<1,POOL,EARLY>".  The launchers dispatch through a table of
 * {key, bf16 kernel, fp16 kernel}, so the key a query reports is the row a launch uses.  Read-only; nothing is launched and
 * no GPU is needed.
 * frmap_conv_plan_key: the key of the launch frmap_conv_igemm (fuse 0 = no residual, 1 = residual), frmap_conv_igemm_ds
 * (fuse 2; K = 3, stride 1; ds_* as there, else ignored) or frmap_conv_igemm_pool2 (fuse 3; K = 3, stride 1) makes for the
 * layer under the tuning, hooks, CU count and batch-invariant flag then in force; pad = K / 2.  The key is copied into buf
 * (n bytes, always terminated) and its length returned; where no plan is taken or the launcher would refuse the layer the
 * answer is "" (0), with the reason in frmap_last_error(); -1 for a fuse out of range.
 * frmap_conv_plan_keys: the number of keys that exist; for 0 <= index < that, key `index` is copied into buf.
 * frmap_conv_plan_selfcheck: 0 when every key selects a plan that has this key, the launch tables hold a kernel of its own
 * for every (key, data type) and no row beyond the keys; else -1 with the first failure in frmap_last_error(). */
int frmap_conv_plan_key(int B, int Hi, int Wi, int Cin, int Cout, int K, int stride, int fuse, int ds_Hi, int ds_Wi, int ds_Cin,
                        int ds_stride, char* buf, int n);
int frmap_conv_plan_keys(int index, char* buf, int n);
int frmap_conv_plan_selfcheck(void);

/* A 3x3 stride-1 pad-1 convolution with a ResNet projection shortcut folded in (BasicBlock.conv2 + bn2 + downsample
 * [conv1x1 stride s + bn] + add + ReLU of the first block of a stage, torchvision resnet.py via face_models.py:67):
 *   out = act( conv3x3(in, W) + conv1x1_stride_s(ds_in, W_ds) + shift ),   shift = shift_conv + shift_shortcut
 *   in        : B×Hi×Wi×Cin;  ds_in : B×ds_Hi×ds_Wi×ds_Cin with (ds_H - 1)/s + 1 == Hi (the block's input)
 *   w_packed  : frmap_pack_conv_weight(W [Cout][Cin][3][3]);  ds_w_packed : frmap_pack_conv_weight(W_ds [Cout][ds_Cin][1][1])
 * The shortcut runs as extra one-tap K stages of the same kernel: no 1x1 launch, no round trip of its output through
 * HBM, no residual read.  frmap_conv_igemm_ds_supported(...) != 0 tells whether a shape takes this kernel (3x3 s1 layers
 * of the register-prefetch kind with ds_Cin <= Cin); otherwise run the shortcut with frmap_conv_igemm and pass it as
 * `residual`. */
int frmap_conv_igemm_ds_supported(int B, int Hi, int Wi, int Cin, int Cout, int ds_Hi, int ds_Wi, int ds_Cin,
                                  int ds_stride);
int frmap_conv_igemm_ds(const void* in, const void* w_packed, const float* shift, const void* ds_in,
                        const void* ds_w_packed, void* out, int B, int Hi, int Wi, int Cin, int Cout,
                        int ds_Hi, int ds_Wi, int ds_Cin, int ds_stride, int relu, int dtype, void* stream);

/* Wide Linear (+folded BatchNorm1d) (+ReLU/GELU `act` as above) (+residual) on the same MFMA kernel:
 *   out[M][N] = act( x[M][K] · Wᵀ + shift [+ residual] ),  x / residual / out in `dtype`, w_packed from
 *   frmap_pack_conv_weight(W as [N][K][1][1]).  When the output has too few tiles to fill the GPU the K
 *   loop is split across workgroups (SiameseNet fc.1, src/face_models.py:148: 18432 -> 1024) and
 *   `workspace` (device, >= frmap_linear_mfma_workspace_bytes(M,K,N) bytes; may be NULL when that is 0)
 *   holds the fp32 partial slabs. */
size_t frmap_linear_mfma_workspace_bytes(int M, int K, int N);
int frmap_linear_mfma(const void* x, const void* w_packed, const float* shift, const void* residual,
                      void* out, void* workspace, int M, int K, int N, int act, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pools (NHWC, `dtype`).
 *   frmap_maxpool        : nn.MaxPool2d(k, s, p)  — (3,2,1) ResNet stem; (2,2,0) BaselineNet /
 *                          SiameseNet (src/face_models.py:27,118,127,136)
 *   frmap_avgpool_global : AdaptiveAvgPool2d(1) -> fp32 B×C (src/face_models.py:30,43; resnet
 *                          avgpool)
 *   frmap_avgpool_adaptive: AdaptiveAvgPool2d((OH,OW)) -> `dtype` B×OH×OW×C
 *                          (src/face_models.py:142), windows [floor(i*H/OH), ceil((i+1)*H/OH))
 * Non-finite input: frmap_maxpool returns NaN for a window that holds a NaN and drops a -inf (nn.MaxPool2d); the average pools
 * return the sum's NaN / inf.  Only the windows that hold the element change.
 * ------------------------------------------------------------------------------------------- */
int frmap_maxpool(const void* in, void* out, int B, int H, int W, int C, int k, int stride, int pad,
                  int dtype, void* stream);
int frmap_avgpool_global(const void* in, float* out_f32, int B, int HW, int C, int dtype, void* stream);
int frmap_avgpool_adaptive(const void* in, void* out, int B, int H, int W, int C, int OH, int OW,
                           int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp32 heads.
 *   frmap_linear_f32 : out[b][n] = [relu]( sum_k x[b][k]*w[n][k] * scale[n] + shift[n] )
 *                      (scale/shift may be NULL = 1/0).  nn.Linear (+ folded BatchNorm1d):
 *                      src/face_models.py:32-33,46-48; :75; :467-468,516-517; :488,580; :678
 *   frmap_l2_normalize_f32 : F.normalize(x, p=2, dim=1, eps) = x / max(||x||, eps)
 *                      (src/face_models.py:179,525,590)
 *   frmap_cast_to_f32 / frmap_cast_from_f32 : dtype <-> fp32 element casts for head glue
 * Non-finite input: frmap_linear_f32's ReLU keeps NaN (relu(-inf) = 0); frmap_l2_normalize_f32 makes a row with a NaN all NaN
 * and a row with an infinity 0 except NaN at the infinity, as F.normalize; the casts keep NaN and the infinities and round a
 * value beyond the range of `dtype` to inf.  Other rows are untouched.
 * ------------------------------------------------------------------------------------------- */
int frmap_linear_f32(const float* x, const float* w, const float* scale, const float* shift,
                     float* out, int B, int K, int N, int relu, void* stream);
int frmap_l2_normalize_f32(const float* x, float* out, int B, int D, float eps, void* stream);
int frmap_cast_to_f32(const void* in, float* out, size_t n, int dtype, void* stream);
int frmap_cast_from_f32(const float* in, void* out, size_t n, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Token-side ops of the hybrid CNN-Transformer (src/face_models.py:618-721), tokens laid out
 * [B][L][D] in `dtype` (= the NHWC trunk output B×7×7×512 viewed as B×49×512).
 *   frmap_add_pos_layernorm : t = x (+ pos[l]) ; y = LayerNorm(t)*gamma+beta (eps)   (:639,644,690)
 *                             t_out (optional) receives t in `dtype`; pos fp32 [L][D] or NULL.
 *   frmap_mha_tokens        : softmax(QK^T/sqrt(128))V per head of nn.MultiheadAttention(512,4)
 *                             (:623,640); qkv = [B][L][3D] as in_proj emits; L <= 64, D = H*128.
 *   frmap_mean_layernorm    : LayerNorm(mean over L tokens) -> fp32 [B][D]               (:718-719)
 * The projections / MLP GEMMs are frmap_conv_igemm calls (K=1, H=W=1) with bias, GELU, residual fused.
 * ------------------------------------------------------------------------------------------- */
int frmap_add_pos_layernorm(const void* x, const float* pos, const float* gamma, const float* beta,
                            void* t_out, void* y_out, int B, int L, int D, float eps, int dtype,
                            void* stream);
int frmap_mha_tokens(const void* qkv, void* out, int B, int L, int D, int H, int dtype, void* stream);
int frmap_mean_layernorm(const void* t, const float* gamma, const float* beta, float* out_f32,
                         int B, int L, int D, float eps, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * AttentionNet's attention block on the trunk map   (/root/reference/src/face_models.py:194-262, GAP :279)
 *   qkv       : [B][H*W][2*Cq + C] (dtype): the 1x1 query | key | value projections (+bias) of x, packed
 *               (one frmap_conv_igemm with the three weight matrices stacked along Cout)
 *   x         : [B][H*W][C] (dtype), the trunk map (NHWC)
 *   gamma     : device float[1]  (AttentionModule.gamma, :220)
 *   spatial_w : device fp32 [2][KS][KS], spatial_b: device float[1]  (SpatialAttention.conv, :199; pad KS/2)
 *   out_map   : [B][H*W][C] (dtype) = (gamma * softmax(q k^T) v + x) * sigmoid(conv([mean_c, max_c]))  or NULL
 *   out_pool  : fp32 [B][C] = mean over the H*W positions of that map (AdaptiveAvgPool2d(1))            or NULL
 *   H*W <= 64, Cq <= 128 (multiple of 8), C in {256, 512}, KS odd.  out_map: 4-byte aligned (stored two channels at a time).
 * ------------------------------------------------------------------------------------------- */
int frmap_cnn_attention(const void* qkv, const void* x, const float* gamma, const float* spatial_w,
                        const float* spatial_b, void* out_map, float* out_pool, int B, int H, int W, int Cq,
                        int C, int KS, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gallery matching (fp32, exact-f32 MFMA).
 *   frmap_match_top1 : for each probe row e (B×D) the FIRST index minimising
 *                      || e - g_i + 1e-6 ||_2 over gallery rows g (G×D) and that distance —
 *                      the batched form of compare_faces' loop (src/app.py:58-63; F.pairwise_distance
 *                      eps semantics).  idx_out int32[B], dist_out fp32[B].  G == 0 -> idx -1,
 *                      dist +inf.  id_or_unknown_out (optional int32[B]) = idx if dist <= thresh else -1
 *                      (compare_faces' "Unknown", src/app.py:64).  packed_out (optional int32[B][2]) =
 *                      {id_or_unknown, bits of dist}: the 8-byte record the multi-GPU all-gather ships.
 *                      The distance is the exact one everywhere: elements (e_i - g_i) + 1e-6 in fp32,
 *                      squares summed in float64, dist = (float)sqrt; a row whose distance is NaN or
 *                      +inf never wins (all rows so: idx -1, dist +inf).
 *                      G <= 64 takes a one-launch exact scan with that arithmetic.  G > 64: a GEMM scores every pair by the
 *                      expanded squared distance WITH a worst-case rounding bound, and every gallery row
 *                      that could be the minimiser within that bound is re-scored with the exact
 *                      ||(e - g) + 1e-6||_2 (float64 accumulation); the first row attaining the exact
 *                      minimum wins.  The index is therefore the reference loop's, not the expanded
 *                      form's (near-duplicate enrolments, un-normalised embeddings included).
 *   frmap_cosine_logits : logits[b][c] = s * <x_b/||x_b||, w_c/||w_c||>  and (optionally)
 *                      argmax_out[b] — class-centre match (src/hyperparameter_tuning.py:1038-1046,
 *                      src/face_models.py:889-893).  logits_out may be NULL.
 *   frmap_arcmargin_eval : ArcMarginProduct.forward in eval mode (src/face_models.py:351-429):
 *                      clamp(cos) -> acos -> target column cos(min(pi-1e-4, theta+m)) (or the
 *                      easy-margin rule) -> * min(s,24) -> NaN/Inf -> 0.  label: int64[B].
 *                      minmax_out (optional) fp32[2] receives max/min raw cosine (:358-360).
 * ------------------------------------------------------------------------------------------- */
/* Evaluation-loop glue (src/testing.py:175-177, 278-279):
 *   frmap_softmax_argmax    : probs = softmax(logits, dim=1) (optional), pred = first arg-max (optional)
 *   frmap_pairwise_distance : dist[b] = ||a_b - b_b + 1e-6||_2 ; same_out[b] = dist < thresh (optional) */
int frmap_softmax_argmax(const float* logits, float* probs_out, int32_t* pred_out, int B, int C, void* stream);
int frmap_pairwise_distance(const float* a, const float* b, float* dist_out, int32_t* same_out, float thresh,
                            int B, int D, void* stream);

/* Classification tally: the accumulate step of the evaluation loop (src/testing.py:278-283) and the counts behind the metric
 * block of src/advanced_metrics.py (per-class precision / recall / F1, the enhanced confusion matrix, expected / maximum
 * calibration error), kept on the device as exact integers.  One launch per batch adds the batch into `state`; nothing is
 * copied or synchronised until the caller reads the state.  The host derives every figure from the integers in float64.
 *
 * The rule, for row i with fp32 logits z[0 .. C) and int32 label y:
 *   declined : y < 0 or y >= C: the row adds 1 to `ignored` and nothing else, whatever its logits are.  Otherwise, if any z[c]
 *              is NaN, +inf or -inf: it adds 1 to `nonfinite` and nothing else.  Row records of a declined row: pred = rank = -1,
 *              conf = loss = NaN.
 *   counted  : pred = the first arg-max (the smallest index among the maxima);
 *              rank = #{c : z[c] > z[y]} + #{c < y : z[c] == z[y]}, so rank == 0 iff pred == y (fp32 comparisons: exact);
 *              conf = 1 / sum_c exp(z[c] - z[pred]) and loss = max(0, log sum_c exp(z[c] - z[pred]) + (z[pred] - z[y])) in fp32:
 *              the device's own values; everything below is defined on their fp32 bits.
 *   bin      : np.digitize(conf, np.linspace(0, 1, n_bins)) - 1, the reference's rule (n_bins EDGES, so only conf == 1.0 falls
 *              in the last bin): edge_k = 1.0 for k == n_bins - 1, else (double)k * (1.0 / (double)(n_bins - 1)); the single edge of
 *              n_bins == 1 is 0; bin = #{k : edge_k <= (double)conf} - 1.
 *   adds     : rows += 1, correct += (rank == 0), loss_q += llrint(min((double)loss, 65536.0) * 2^24);
 *              rank_hist[min(rank, R - 1)] += 1; support[y] += 1, predicted[pred] += 1, hit[y] += (rank == 0);
 *              bin_count[b] += 1, bin_correct[b] += (rank == 0), bin_conf_q[b] += llrint((double)conf * 2^32);
 *              confusion[y * C + pred] += 1 with keep_confusion.
 *   Integer adds only (64-bit atomics): a state holds the same bits for any order of the rows and any split into launches.
 * state : uint64 words, zeroed by the caller before the first launch: an 8-word header (rows, ignored, nonfinite, correct, loss_q,
 *         three reserved words that stay zero), then rank_hist[R], support[C], predicted[C], hit[C], bin_count[n_bins],
 *         bin_correct[n_bins], bin_conf_q[n_bins] and, with keep_confusion, confusion[C * C].  The words-query takes no stream,
 *         returns the number of WORDS, and 0 for arguments the launcher would refuse.  loss_q reaches 2^64 after 2^24 rows at the
 *         clamp and after 2^34 rows of losses below 64; bin_conf_q after 2^32 rows.
 * Refused (-1, the text names the argument): B < 1 or above 2^26 - 4 (one wavefront per row); C < 1; R or n_bins outside
 * 1 ... 1024; keep_confusion with C > 4096 (the matrix alone would be 128 MiB of state).
 * logits [B][C] fp32, labels [B] int32; row_pred_out / row_rank_out int32 [B] and row_conf_out / row_loss_out fp32 [B] are optional
 * (NULL skips them).  Every pointer is walked element by element: logits, labels and the four row outputs need their element size
 * (4), state the size of a uint64 counter (8).
 * The host form is the same accumulation compiled for the CPU (host pointers, no stream, B = 0 allowed): it computes pred and rank
 * from the logits itself, while row_conf_host and row_loss_host are INPUTS - the device's own values, so that the two states can be
 * compared word for word; it refuses a counted row whose conf is outside [0, 1] or whose loss is negative or NaN, with the
 * state untouched. */
size_t frmap_classify_tally_words(int C, int R, int n_bins, int keep_confusion);
int frmap_classify_tally(const float* logits, const int32_t* labels, int B, int C, int R, int n_bins, int keep_confusion,
                         uint64_t* state, int32_t* row_pred_out, int32_t* row_rank_out, float* row_conf_out, float* row_loss_out,
                         void* stream);
int frmap_classify_tally_host(const float* logits_host, const int32_t* labels_host, int B, int C, int R, int n_bins,
                              int keep_confusion, uint64_t* state_host, int32_t* row_pred_host, int32_t* row_rank_host,
                              const float* row_conf_host, const float* row_loss_host);

/* One-vs-rest rank counts: the exact one-vs-rest ROC AUC and average precision of the reference's metric block
 * (src/testing.py:296-312: roc_auc_score(multi_class='ovr'), average_precision_score) and the per-class roc_auc of
 * src/advanced_metrics.py:85-100, without a sort and without a copy of the scores to the host.  Every batch is appended to a
 * score store on the device; one count at the end gives every row three exact integers, from which the host derives both
 * curves' areas in float64 (evaluate.ovr_metrics).
 *
 * The score store, caller-owned: store = fp32 [C][capacity], CLASS-MAJOR (the count streams column c for all positives of c, and
 * that read must be contiguous); store_labels = int32 [capacity].  capacity and first are 64-bit and all index arithmetic is.
 * frmap_ovr_append writes rows [first, first + B): store[c * capacity + first + b] = scores[b][c] (transposed through LDS: the
 * read and the write are both coalesced) and store_labels[first + b] =
 *   the label : if it lies in [0, C) and every score of the row is finite;
 *   -1        : for a label outside [0, C), whatever the scores are;
 *   -2        : for a NaN, +inf or -inf among the scores of a row whose label is in range.
 * These are the two kinds of declined row of frmap_classify_tally, so rows / ignored / nonfinite agree with a tally fed the same
 * batches.  Nothing outside rows [first, first + B) of the C columns and of the labels is written.
 * Refused (-1, the text names the argument): B < 1 or above 2^26 - 4; C < 1; first < 0; first + B > capacity.
 *
 * frmap_ovr_rank_counts, over rows [0, n) of the store.  A row with a stored label in [0, C) is COUNTED.  A counted row i is a
 * positive of exactly one class, y_i; with s_i = store[y_i][i], over the counted rows j < n (j == i included):
 *   ge_same[i]  = #{ j : y_j == y_i and store[y_i][j] >= s_i }      (>= 1)
 *   ge_other[i] = #{ j : y_j != y_i and store[y_i][j] >= s_i }
 *   eq_other[i] = #{ j : y_j != y_i and store[y_i][j] == s_i }
 * A declined row gets 0, 0, 0 and takes part in nobody's count.  The comparisons are IEEE fp32 comparisons made AS FLOATS WITH
 * DENORMALS HONOURED (no integer key): -0.0 equals +0.0, a denormal is not zero, NaN compares false.  With P_c positives and
 * N_c = rows - P_c negatives of class c, in float64 on the host:
 *   roc_auc[c]           = (sum_{i in c} (N_c - ge_other[i]) + 1/2 sum_{i in c} eq_other[i]) / (P_c N_c)
 *   average_precision[c] = (sum_{i in c} ge_same[i] / (ge_same[i] + ge_other[i])) / P_c
 * - the Mann-Whitney form of the trapezoid under roc_curve with ties at one half, and sklearn's step-wise sum.
 * ge_same_out / ge_other_out / eq_other_out: uint64 [n] each.  The call writes every word of [0, n) itself (one kernel that zeroes,
 * then one kernel that adds with 64-bit integer atomics; no floating-point atomic): the caller does not pre-zero them.  Exact
 * integers: the same store gives the same words on every run, whatever the split into appends; rows in another order give the
 * same integers per row.  n^2 comparisons whatever C is.  No scratch, nothing allocated or synchronised.
 * Refused (-1, the text names the argument): n < 1 or above 2^31 - 1; n > capacity; C < 1 or above 2^24 - 1 (one workgroup per
 * class and segment).
 * Every pointer is walked element by element: scores, labels, store and store_labels need their element size (4), ge_same_out,
 * ge_other_out and eq_other_out the size of a uint64 counter (8).
 * The host form is the same count compiled for the CPU (host pointers, no stream, n = 0 allowed). */
int frmap_ovr_append(const float* scores, const int32_t* labels, int B, int C, float* store, int32_t* store_labels,
                     long long capacity, long long first, void* stream);
int frmap_ovr_rank_counts(const float* store, const int32_t* store_labels, long long n, long long capacity, int C,
                          uint64_t* ge_same_out, uint64_t* ge_other_out, uint64_t* eq_other_out, void* stream);
int frmap_ovr_rank_counts_host(const float* store_host, const int32_t* store_labels_host, long long n, long long capacity, int C,
                               uint64_t* ge_same_host, uint64_t* ge_other_host, uint64_t* eq_other_host);

/* Head fitting: one training step of a linear softmax classifier (the nn.Linear(512, C) of ResNetTransfer's frozen phase, of
 * two-phase ArcFace training and of src/testing.py:134-136) over CACHED trunk features.  Softmax regression on a [B, D] view of a
 * cached [N, D] matrix with a torch.optim.Adam / AdamW update: one small memset and three launches on the caller's stream,
 * nothing copied to the host, nothing allocated.  No backward pass through a trunk exists here.
 *
 * Operands: x [N][D] fp32, labels [N] int32, rows [B] int32 (indices into x and labels; NULL: rows 0 .. B-1 - a mini-batch is a
 * view of the cache), keep [B][D] uint8 or NULL (a dropout mask over the batch rows) with keep_scale = 1 / (1 - p), w [C][D] and
 * b [C] fp32, updated in place.  flags: 1 = decoupled weight decay (AdamW; else the coupled L2 of Adam), 2 = AMSGrad, 4 = clear
 * the epoch figures first.
 * The rule:
 *   x'       = keep ? (keep[i][k] ? x * keep_scale : 0) : x, one rounding
 *   declined : a batch row whose rows entry is outside [0, N), whose label is outside [0, C) or any of whose D features is NaN or
 *              an infinity contributes nothing; n counts the others, on the device.  n == 0 changes no weight and no moment and
 *              does not advance t.
 *   z = x' w^T + b;  p = softmax(z), max-subtracted;  y = (1 - ls) onehot + ls / C;  row loss = -sum y log p;  g = (p - y) / n:
 *   the softmax, the loss and g are evaluated in float64 from the fp32 logits and rounded to fp32 once;
 *   dw = g^T x', db = sum over the rows of g;  then Adam / AdamW with the bias corrections of step t, every operation fp32 and
 *   rounded once (fmaf where torch fuses: lerp_, addcmul_, addcdiv_).
 *   Summation order: every dot product (length D forward, length B backward) is cut at the multiples of 128; a chain is fmaf from
 *   +0 in ascending k, the chains are added in ascending order from +0, the bias last.  The fp32-input MFMA of gfx950 is that fmaf
 *   chain bit for bit, so full 32 x 32 tiles run on the matrix cores and ragged edges on plain fmaf lanes with the same bits;
 *   nothing depends on the grid or the device.  The same operands give the same bits on every run: no floating-point atomic.
 * state : frmap_head_fit_state_bytes bytes, zeroed by the caller before the first step: eight uint64 words - t, n of the last step,
 *         and the epoch figures rows, correct, loss_q (the tally's fixed point: clamp 65536, scale 2^24), three reserved - then fp32
 *         m_w [C][D], v_w [C][D], m_b [C], v_b [C] and, sized for AMSGrad, vmax_w [C][D], vmax_b [C].  t lives here, so a captured
 *         step replays correctly.
 * workspace : exactly frmap_head_fit_workspace_bytes bytes: fp32 z [B][C], g [B][C], row_loss [B] (NaN for a declined row, whose
 *         rows of z and g are +0), int32 row_src [B] (the row of x read, -1 for a declined row).  D does not enter the size.
 * The size queries take no stream and return 0 for arguments the launcher would refuse.
 * Refused (-1, the text names the argument): N < 1; B < 1 or above 2^20; D < 1 or above 65536; C < 1 or above 65536 (one
 * wavefront per row of the softmax; the grid of the update); unknown flag bits.
 * Every pointer is walked element by element: x, labels, rows, w, b and workspace need their element size (4), keep 1, state the
 * size of a uint64 counter (8).
 * The host form is the same step compiled for the CPU (host pointers, no stream; its workspace holds the same z, g, row_loss and
 * row_src).  With given_g != 0 the z, g and row_loss of the workspace are INPUTS - the device's own, whose exp / log are not the
 * C library's - and the figures, dw, db and the update are computed from them, so that weights and moments can be compared with
 * the device's word for word. */
size_t frmap_head_fit_state_bytes(int D, int C, int amsgrad);
size_t frmap_head_fit_workspace_bytes(int B, int D, int C);
int frmap_head_fit_step(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale, float* w,
                        float* b, void* state, void* workspace, int N, int B, int D, int C, float lr, float beta1, float beta2,
                        float eps, float weight_decay, float label_smoothing, int flags, void* stream);
int frmap_head_fit_step_host(const float* x_host, const int32_t* labels_host, const int32_t* rows_host, const uint8_t* keep_host,
                             float keep_scale, float* w_host, float* b_host, void* state_host, void* workspace_host, int N, int B,
                             int D, int C, float lr, float beta1, float beta2, float eps, float weight_decay, float label_smoothing,
                             int flags, int given_g);

/* Head fitting in groups: H independent heads over ONE cache advanced by one call - the folds of a cross-validation, the trials
 * of a parameter sweep.  Head h of a grouped step has exactly the bits of frmap_head_fit_step run on head h's slices alone: the
 * rule, the 128-long chains and the tile code are the single step's; the head is the slowest dimension of every grid.
 * Shared by all heads: x [N][D], labels [N].  Per head, H single-head operands back to back: rows [H][B] (required: an entry
 * outside [0, N), -1 say, declines that batch row - the padding of a head with fewer rows than B), keep [H][B][D] or NULL for all
 * heads, w [H][C][D], b [H][C], the states frmap_head_fit_group_state_stride bytes apart (the single size rounded up to a multiple
 * of 8, so that every head's uint64 header is 8-aligned; padding bytes are neither read nor written), the workspaces
 * frmap_head_fit_workspace_bytes apart.
 * hyper [H][8] fp32 in DEVICE memory: lr, beta1, beta2, eps, weight_decay, label_smoothing, keep_scale, 0.  The kernels read a
 * head's row where the single step takes its scalars by value (the same fp32 values give the same bits), so a learning rate is
 * changed by writing the table on the stream and a captured step replays with what the table holds at replay time.
 * flags: 1, 2 and 4 as in the single step, for the whole group (2 decides the state size); 8 = evaluate only: logits, softmax and
 * figures - every head's n is written and its rows, correct and loss_q are added to; t, w, b and the moments are not touched - and
 * keep must be NULL.  The figures a training step adds are those of its weights BEFORE the update, so an evaluate call adds what a
 * training step on a copy of the head would.
 * Launches: one small kernel that zeroes every head's n (with 4: its three figures too) - no memset nodes -, then the three kernels
 * of the single step (two with flag 8).  A head whose rows are all declined changes nothing of its own and keeps its t while its
 * neighbours proceed.
 * Refused (-1, the text names the argument): H outside [1, 4096]; the single step's limits on N, B, D, C; rows or hyper NULL;
 * flag bits above 15; keep with flag 8.  The size queries return 0 for arguments the launcher would refuse.
 * x, labels, rows, hyper, w, b and workspace need their element size (4), keep 1, state the size of a uint64 counter (8).
 * The host form loops the single host step over the heads with the same stride and table (host pointers, flag 8 included);
 * given_g means per head what it means there. */
size_t frmap_head_fit_group_state_stride(int D, int C, int amsgrad);
size_t frmap_head_fit_group_state_bytes(int H, int D, int C, int amsgrad);
size_t frmap_head_fit_group_workspace_bytes(int H, int B, int D, int C);
int frmap_head_fit_group_step(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, const float* hyper,
                              float* w, float* b, void* state, void* workspace, int N, int H, int B, int D, int C, int flags,
                              void* stream);
int frmap_head_fit_group_step_host(const float* x_host, const int32_t* labels_host, const int32_t* rows_host, const uint8_t* keep_host,
                                   const float* hyper_host, float* w_host, float* b_host, void* state_host, void* workspace_host,
                                   int N, int H, int B, int D, int C, int flags, int given_g);

/* Head fitting with one hidden layer: one training step of Linear(D, Hd) -> ReLU -> dropout -> Linear(Hd, C) (the fc1 / fc2 of the
 * reference's BaselineNet, src/face_models.py:16-60; a learned projection on any other cached feature) over CACHED trunk features:
 * plain backpropagation through one ReLU with one Adam / AdamW optimiser over the four tensors.  One small memset and six launches
 * on the caller's stream, nothing copied to the host, nothing allocated, no floating-point atomic.
 *
 * Operands: x, labels and rows as in frmap_head_fit_step; keep1 [B][D] uint8 or NULL with keep1_scale masks the input, keep2
 * [B][Hd] uint8 or NULL with keep2_scale the hidden layer; w1 [Hd][D], b1 [Hd], w2 [C][Hd], b2 [C] fp32, updated in place.
 * flags: 1 | 2 | 4 as in the single step.
 * The rule (every dot product is the single step's: fmaf chains from +0 cut at the multiples of 128, the chains added ascending):
 *   x'       = keep1 ? (keep1[i][k] ? x * keep1_scale : 0) : x, one rounding
 *   a[i][j]  = dot_k(x'[i][k], w1[j][k]) + b1[j]                     (chain order over D, the bias last)
 *   h[i][j]  = a > 0 ? a : (a != a ? a : +0)                         (a NaN stays one; -0 and negatives give +0)
 *   lab[i]   = labels[rows[i]], or -1 where layer 1 declines row i (row index outside [0, N), label outside [0, C), a non-finite
 *              feature); the h row of such a row is +0
 *   layer 2  = the forward half of frmap_head_fit_step on (x := h [B][Hd], labels := lab [B], rows := NULL, keep := keep2, w2, b2):
 *              z, the float64 softmax, the row loss, g = (p - y) / n and the figures.  It declines a row whose lab is -1 or whose
 *              h holds a non-finite value; n is ITS count, the one n of the step.
 *   s[i][j]  = dot_c(g[i][c], w2[c][j])                              (chain order over C, w2 BEFORE its update)
 *   da[i][j] = (row i counted by layer 2) && h[i][j] > 0 && keep2[i][j] ? s * keep2_scale : +0, one rounding (no mask: s itself)
 *   dw2, db2 = the single step's on (g, h');  dw1[j][d] = dot_i(da[i][j], x'[i][d]), db1[j] = dot_i(da[i][j], 1)
 *   update   = Adam / AdamW on all four tensors with the same hyper-parameters and the same t.  n == 0 changes nothing but the
 *              workspace.
 * Launches: the memset of layer 2's n (with 4: its figures); layer 1 forward (the logits tile walk with the ReLU epilogue: h, lab,
 * row_src1); the single step's logits and softmax kernels on (h, lab); back (da, a workgroup per 32 x 32 tile over all C, on the
 * matrix cores where the tile is full; one thread copies t and n into layer 1's state); the single step's update kernel on layer 2,
 * then on layer 1 with g := da.  w2 is not updated before da is written: the stream order gives that.
 * state : frmap_head_fit_hidden_state_bytes bytes, zeroed by the caller before the first step: the single step's layout for
 *         (D, Hd), then the single step's layout for (Hd, C); both are multiples of 8.  The second part is a valid state of
 *         frmap_head_fit_step on (h, lab): its header carries t, n and the epoch figures.  The first part's t and n are copies
 *         written by the step; its figure words stay 0.
 * workspace : exactly frmap_head_fit_hidden_workspace_bytes bytes: fp32 h [B][Hd], da [B][Hd], int32 lab [B], row_src1 [B], then
 *         the single step's workspace for (B, Hd -> C).
 * The size queries take no stream and return 0 for arguments the launcher would refuse.
 * Refused (-1, the text names the argument): N < 1; B < 1 or above 2^20; D, Hd or C < 1 or above 65536; flag bits above 7; a
 * required pointer that is NULL.  All address arithmetic is size_t.
 * Every pointer is walked element by element: x, labels, rows, w1, b1, w2, b2 and workspace need their element size (4), keep1
 * and keep2 1, state the size of a uint64 counter (8).
 * The host form is the same step compiled for the CPU (host pointers, no stream); given_g != 0 takes z, g and row_loss of the
 * layer-2 workspace as INPUTS, as in frmap_head_fit_step_host. */
size_t frmap_head_fit_hidden_state_bytes(int D, int Hd, int C, int amsgrad);
size_t frmap_head_fit_hidden_workspace_bytes(int B, int D, int Hd, int C);
int frmap_head_fit_hidden_step(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep1, float keep1_scale,
                               const uint8_t* keep2, float keep2_scale, float* w1, float* b1, float* w2, float* b2, void* state,
                               void* workspace, int N, int B, int D, int Hd, int C, float lr, float beta1, float beta2, float eps,
                               float weight_decay, float label_smoothing, int flags, void* stream);
int frmap_head_fit_hidden_step_host(const float* x_host, const int32_t* labels_host, const int32_t* rows_host, const uint8_t* keep1_host,
                                    float keep1_scale, const uint8_t* keep2_host, float keep2_scale, float* w1_host, float* b1_host,
                                    float* w2_host, float* b2_host, void* state_host, void* workspace_host, int N, int B, int D, int Hd,
                                    int C, float lr, float beta1, float beta2, float eps, float weight_decay, float label_smoothing,
                                    int flags, int given_g);

/* Head fitting on pairs: one training step of a contrastive head x -> normalize(x w^T + b) over PAIRS of cached rows - the objective
 * of the reference's Siamese family (ContrastiveLoss(margin 2.0, pos_weight 1.2, neg_weight 0.8), src/face_models.py:725-774) with the
 * trunk frozen; for a SiameseNet w and b are its own last layer fc.8.  One small memset and four launches on the caller's stream,
 * nothing copied to the host, nothing allocated, no floating-point atomic.
 *
 * Operands: x [N][D] fp32 (the cache); left [P], right [P] int32 rows of x; differ [P] int32: 0 = the same identity (pulled
 * together), 1 = different identities (pushed apart up to margin) - the loss's own meaning of its label (the reference's
 * SiameseDataset hands it 1 for SAME-class pairs; callers here derive differ from identity labels); keep [2P][D] uint8 or NULL with
 * keep_scale (a dropout mask over the 2P batch rows); w [E][D], b [E] fp32, updated in place; margin, w_same (the weight of a
 * differ = 0 pair), w_diff (of a differ = 1 pair), accept (the distance below which a pair counts as accepted in the figures).
 * flags: 1 | 2 | 4 as in frmap_head_fit_step.
 * The rule (dot products are the single step's: fmaf chains from +0 cut at the multiples of 128, the chains added ascending):
 *   batch    : 2P rows; row i < P reads left[i], row P + i reads right[i].  A row whose index is outside [0, N) or any of whose D
 *              features is NaN or an infinity is declined.
 *   a[i][e]  = dot_k(x'[i][k], w[e][k]) + b[e], the bias last; the a row of a declined row is +0
 *   counted  : pair p is counted iff both of its rows are and differ[p] is 0 or 1; n counts them, on the device.  An uncounted pair
 *              has row_src = -1 on both its rows, +0 rows of ga and NaN in pair_loss and dist.  n == 0 changes no weight and no
 *              moment and does not advance t.
 *   per counted pair, in float64 from the fp32 a and rounded to fp32 once:
 *              s = max(||a||, 1e-12), u = a_l / s_l, v = a_r / s_r;  delta = (u - v) + 1e-6, d0 = ||delta||, d = max(d0, 1e-8)
 *              pair_loss = differ ? w_diff max(margin - d, 0)^2 : w_same d^2;  dist = d
 *              q = (differ ? -2 w_diff max(margin - d, 0) : 2 w_same d) / n, 0 where d0 < 1e-8;  gd = q delta / d0
 *              ga_l = (gd - u (u . gd)) / s_l where ||a_l|| > 1e-12, else gd / 1e-12;  ga_r the same with -gd and v
 *   figures  : rows += n, correct += #((dist < accept) == (differ == 0)) on the fp32 dist, loss_q += the fixed point of pair_loss
 *   update   : dw = ga^T x' over the 2P rows, db = sum ga, Adam / AdamW: the single step's update with B := 2P, C := E.
 * Launches: the memset of n (with 4: the figures); forward (the logits tile walk, identity epilogue, no labels: a, row_src); gate
 * (a thread per pair: marks uncounted pairs, one integer atomic per wavefront into n); pair (a wavefront per pair: float64 wavefront
 * sums, ga, pair_loss, dist; at most two integer atomics per workgroup; advances t when n > 0); the single step's update kernel.
 * state : frmap_head_fit_pair_state_bytes bytes = the single step's layout for (D, E), zeroed by the caller before the first step.
 * workspace : exactly frmap_head_fit_pair_workspace_bytes bytes: fp32 a [2P][E], ga [2P][E], pair_loss [P], dist [P], int32
 *         row_src [2P].  D does not enter the size.
 * The size queries take no stream and return 0 for arguments the launcher would refuse.
 * Refused (-1, the text names the argument): N < 1; P < 1 or above 2^19 (2P batch rows); D or E < 1 or above 65536; flag bits above
 * 7; a required pointer that is NULL.
 * Every pointer is walked element by element: x, left, right, differ, w, b and workspace need their element size (4), keep 1,
 * state the size of a uint64 counter (8).
 * The host form is the same step compiled for the CPU (host pointers, no stream); given_g != 0 takes a, ga, pair_loss and dist of the
 * workspace as INPUTS - the device's own - and computes row_src, n, the figures, dw, db and the update from them. */
size_t frmap_head_fit_pair_state_bytes(int D, int E, int amsgrad);
size_t frmap_head_fit_pair_workspace_bytes(int P, int D, int E);
int frmap_head_fit_pair_step(const float* x, const int32_t* left, const int32_t* right, const int32_t* differ, const uint8_t* keep,
                             float keep_scale, float* w, float* b, void* state, void* workspace, int N, int P, int D, int E,
                             float margin, float w_same, float w_diff, float accept, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int flags, void* stream);
int frmap_head_fit_pair_step_host(const float* x_host, const int32_t* left_host, const int32_t* right_host, const int32_t* differ_host,
                                  const uint8_t* keep_host, float keep_scale, float* w_host, float* b_host, void* state_host,
                                  void* workspace_host, int N, int P, int D, int E, float margin, float w_same, float w_diff,
                                  float accept, float lr, float beta1, float beta2, float eps, float weight_decay, int flags,
                                  int given_g);

/* Head fitting with a margin: one training step of the class centres w [C][D] of an ArcFace margin head (the reference's
 * ArcMarginProduct, src/face_models.py:297-429) under softmax cross-entropy with the trunk frozen - the weight that
 * frmap_cosine_logits scores against.  One small memset and four launches on the caller's stream, nothing copied to the host, nothing
 * allocated, no floating-point atomic.
 *
 * Operands: x, labels, rows, keep / keep_scale as in frmap_head_fit_step (the cache should hold the model's embeddings); w [C][D]
 * fp32, updated in place; there is no bias.  s, m: the EFFECTIVE scale and margin of this step (the reference's warm-up schedule is
 * host arithmetic: head_fit.margin_schedule).  flags: 1 | 2 | 4 as in frmap_head_fit_step, 16 = easy margin.
 * The rule (dot products are the single step's chains; declined rows are the single step's):
 *   z[i][c]  = dot_k(x'[i][k], w[c][k]); the z row of a declined row is +0
 *   rx[i]    = fp32(1 / max(||x'_i||, 1e-12)), rw[c] = fp32(1 / max(||w_c||, 1e-12)), the squared norms summed in float64; rx of a
 *              declined row is +0.  From here in float64 on the fp32 z, rx, rw, rounded to fp32 once:
 *   cos      = (z rx[i]) rw[c];  cs = clamp(cos, -HI, HI), inside = -HI <= cos <= HI, HI = fp32(1 - 1e-7)
 *   target   : theta = acos(cs); theta + m >= CAP = fp32(pi - 1e-4) ? out = cos(CAP), dfac = 0
 *              : out = cos(theta + m), dfac = inside sin(theta + m) / sin(theta).  Easy margin: cs > 0 ? the margin branch (no cap)
 *              : out = cs, dfac = inside.
 *   others   : out = cs, dfac = inside
 *   l = s out; softmax, row loss (label smoothing as in the single step), pred = the first arg-max of l
 *   q = s (p - y) / n;  g[i][c] = fp32(q dfac rx[i]);  h[i][c] = fp32(q dfac cos);  cosv[i][c] = fp32(cs)
 *   dw[c][d] = rw[c] dot_i(g[i][c], x'[i][d]) - rw[c]^2 dot_i(h[i][c], 1) w[c][d], every product and the difference rounded once; the
 *              second term is absent where rw[c] is not below fp32(1e12) (a clamped norm)
 *   update   : Adam / AdamW on w as in the single step; figures as in the single step; n == 0 changes nothing but the workspace.
 * Launches: the memset of n (with 4: the figures); logits (the tile walk without a bias: z, row_src, n); norms (a wavefront per row
 * of the batch and of w: rx, rw; independent of the launch before); margin softmax (a wavefront per row: cosv, g, h, row_loss, the
 * figures; advances t when n > 0); update (a 32 x 32 tile of w per workgroup: both chains over B, the combination, Adam).
 * state : frmap_head_fit_margin_state_bytes bytes = the single step's layout for (D, C) (the bias moments stay zero), zeroed by the
 *         caller before the first step.
 * workspace : exactly frmap_head_fit_margin_workspace_bytes bytes: fp32 z [B][C], cosv [B][C], g [B][C], h [B][C], row_loss [B],
 *         rx [B], rw [C], int32 row_src [B].  D does not enter the size.
 * The size queries take no stream and return 0 for arguments the launcher would refuse.
 * Refused (-1, the text names the argument): N < 1; B < 1 or above 2^20; D or C < 1 or above 65536; flag bits outside 1 | 2 | 4 | 16; a
 * required pointer that is NULL (rows and keep may be).
 * Every pointer is walked element by element: x, labels, rows, w and workspace need their element size (4), keep 1, state the size
 * of a uint64 counter (8).
 * The host form is the same step compiled for the CPU (host pointers, no stream); given_g != 0 takes z, cosv, g, h, row_loss, rx and
 * rw of the workspace as INPUTS - the device's own - and computes row_src, n, the figures, dw and the update from them. */
size_t frmap_head_fit_margin_state_bytes(int D, int C, int amsgrad);
size_t frmap_head_fit_margin_workspace_bytes(int B, int D, int C);
int frmap_head_fit_margin_step(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale, float* w,
                               void* state, void* workspace, int N, int B, int D, int C, float s, float m, float label_smoothing, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int flags, void* stream);
int frmap_head_fit_margin_step_host(const float* x_host, const int32_t* labels_host, const int32_t* rows_host, const uint8_t* keep_host,
                                    float keep_scale, float* w_host, void* state_host, void* workspace_host, int N, int B, int D, int C,
                                    float s, float m, float label_smoothing, float lr, float beta1, float beta2, float eps,
                                    float weight_decay, int flags, int given_g);

/* Head fitting of an embedding layer: one training step of x -> x w1^T -> BatchNorm1d (TRAINING mode) -> dropout -> normalize ->
 * ArcMarginProduct -> cross-entropy with the trunk frozen - the `embedding`, `bn` and `arcface` tensors of the reference's ArcFaceNet
 * under one optimiser, the first phase of its two-phase training (src/training.py:374-377, 683-700, src/face_models.py:492-498,
 * 511-535) - over cached POOLED trunk features.  One small memset and ten launches on the caller's stream, nothing copied to the
 * host, nothing allocated, no floating-point atomic.
 *
 * Operands: x, labels, rows as in frmap_head_fit_step (the cache should hold the pooled trunk features); keep [B][E] uint8 or NULL
 * with keep_scale: the dropout BEHIND the BatchNorm; w1 [E][D] (no bias), gamma, beta, running_mean, running_var [E] and the class
 * centres wc [C][E], all fp32 and updated in place; bn_eps, bn_momentum: BatchNorm1d's; s, m: the effective scale and margin as in
 * frmap_head_fit_margin_step.  flags: 1 | 2 | 4 | 16 as there.
 * The rule (dot products are the single step's chains; layer 1 declines rows as the single step does, n1 remain):
 *   a[i][j]  = dot_k(x[i][k], w1[j][k]); a declined row is +0
 *   per column over the n1 counted rows, in float64 from the fp32 a: mean, var = sum (a - mean)^2 / n1 (two passes);
 *              mean32 = fp32(mean), rstd = fp32(1 / sqrt(var + bn_eps)), uvar = fp32(var n1 / (n1 - 1)); all +0 where n1 < 2
 *   ah       = fp32((a - mean32) rstd) in float64 on the fp32 bits;  y = fl(fl(gamma ah) + beta);  y' = kept ? fl(y keep_scale) : +0
 *   margin   : frmap_head_fit_margin_step's forward half on (x := y', labels := lab, rows := NULL, keep := NULL, w := wc), bit for
 *              bit; its count is n2
 *   taken    : iff n1 >= 2 and n2 == n1.  A step that is not taken writes the workspace and nothing else - no parameter, moment,
 *              running statistic, epoch figure or step count moves (bit 4 still clears the figures); word n of the headers is 0.
 *   gy       = gate (S - rx^2 k y'), S = dot_c(fl(g rw[c]), wc[c][e]) with wc before its update, k = dot_c(h, 1), every product and
 *              the difference rounded once; the second term is absent where rx is not below fp32(1e12)
 *   dbeta    = dot_i(gy, 1), dgamma = dot_i(gy, ah);  da = fp32((gamma rstd) ((gy - dbeta / n1) - ah (dgamma / n1))) in float64
 *   dw1      = dot_i(da[i][j], x[i][d]);  dwc = the margin step's own
 *   update   : Adam / AdamW on w1, gamma, beta and wc with one t;  running_mean = fl(fl((1 - mom) rm) + fl(mom mean32)), running_var
 *              likewise with uvar.
 * state : frmap_head_fit_embed_state_bytes bytes, zeroed by the caller before the first step: the single step's layout for (D, E),
 *         for (1, E) (gamma as the weight, beta as the bias) and for (E, C), each a multiple of 8.  The last part is a valid state of
 *         frmap_head_fit_margin_step for the centres: its header carries t, n and the epoch figures.
 * workspace : exactly frmap_head_fit_embed_workspace_bytes bytes: fp32 a, ah, y', gy, da [B][E], mean32, rstd, uvar, dbeta, dgamma
 *         [E], int32 lab [B], row_src1 [B], n1 and one padding word, then the margin workspace for (B, C).  D does not enter the size.
 * The size queries take no stream and return 0 for arguments the launcher would refuse.
 * Refused (-1, the text names the argument): N < 1; B < 1 or above 2^20; D, E or C < 1 or above 65536; flag bits outside
 * 1 | 2 | 4 | 16; a required pointer that is NULL (rows and keep may be).
 * Every pointer is walked element by element: x, labels, rows, w1, gamma, beta, running_mean, running_var, wc and workspace need
 * their element size (4), keep 1, state the size of a uint64 counter (8).
 * The host form is the same step compiled for the CPU (host pointers, no stream).  `given` is a bit mask of the float64 stages whose
 * outputs in the workspace are INPUTS - the device's own: 1 = mean32, rstd, uvar and ah; 2 = the margin stage (z, cosv, g, h, row_loss,
 * rx, rw, as given_g of frmap_head_fit_margin_step_host); 4 = da.  Other bits are refused. */
size_t frmap_head_fit_embed_state_bytes(int D, int E, int C, int amsgrad);
size_t frmap_head_fit_embed_workspace_bytes(int B, int D, int E, int C);
int frmap_head_fit_embed_step(const float* x, const int32_t* labels, const int32_t* rows, const uint8_t* keep, float keep_scale, float* w1,
                              float* gamma, float* beta, float* running_mean, float* running_var, float* wc, void* state, void* workspace,
                              int N, int B, int D, int E, int C, float bn_eps, float bn_momentum, float s, float m, float label_smoothing,
                              float lr, float beta1, float beta2, float eps, float weight_decay, int flags, void* stream);
int frmap_head_fit_embed_step_host(const float* x_host, const int32_t* labels_host, const int32_t* rows_host, const uint8_t* keep_host,
                                   float keep_scale, float* w1_host, float* gamma_host, float* beta_host, float* running_mean_host,
                                   float* running_var_host, float* wc_host, void* state_host, void* workspace_host, int N, int B, int D,
                                   int E, int C, float bn_eps, float bn_momentum, float s, float m, float label_smoothing, float lr,
                                   float beta1, float beta2, float eps, float weight_decay, int flags, int given);

/* Scratch frmap_cosine_logits / frmap_arcmargin_eval need (device, caller-owned, >= this many bytes, 16-byte
 * aligned). */
size_t frmap_head_workspace_bytes(int B, int C);
/* Scratch of frmap_match_top1 and frmap_match_top1_packed for B probes against G gallery rows (candidate records +
 * row statistics; device, caller-owned, 16-byte aligned). */
size_t frmap_match_workspace_bytes(int B, int G);
int frmap_match_top1(const float* emb, const float* gallery, int32_t* idx_out, float* dist_out,
                     int32_t* id_or_unknown_out, int32_t* packed_out, float thresh, void* workspace,
                     int B, int G, int D, void* stream);
/* The same match for LARGE galleries on the fp16 MFMA pipe (same outputs, same contract, same exact re-scoring of
 * every in-band candidate).  Every fp32 operand is split into two fp16
 * numbers (hi = fp16(S x), lo = fp16(S x - hi)); one K = 3 D GEMM accumulates a_hi.g_hi + a_hi.g_lo + a_lo.g_hi in
 * fp32 (the fp32 dot product to ~2^-22).  frmap_match_pack_gallery prepares a gallery ONCE: packed_out
 * (frmap_match_gallery_pack_bytes(G, D) bytes) and stat_w_out [G][4]; D % 32 == 0.  Each row is scaled by its own power
 * of two S before the split (csrc/match_scale_rule.h).  Magnitude range: every finite fp32 row, subnormals and the zero row
 * included, alone or mixed with any other in one call, gets the documented exact answer.  S, 1 / S and every fp16 element of the
 * pack are finite for every row; 1 / S is a normal power of two.  A row whose largest |x| is at least the cut 2^-113 has it scaled
 * into [2^13, 2^14); below the cut S stays at 2^126 and the row's low halves lose bits, an error far inside the rounding bound the
 * epilogue already allows.  Past the overflow of an fp32 squared norm (a row norm above about 1.8e19, 2^64) the expanded distance of
 * every pair of that row has no finite bound: such a pair is kept as a candidate by every epilogue (top-1, top-k, verification
 * counts, threshold search) and decided by its exact distance, which is finite as long as the fp32 differences are (|e_i - g_i| up
 * to FLT_MAX) and reported as long as its fp32 cast is; calls dominated by such rows run at the speed of the exact scan.  The
 * unpacked entry points give the same answers over the same range.  The packer writes packed_out element by element (2-byte aligned serves
 * there; every call that reads the pack needs it and stat_w 16-byte aligned).  frmap_match_top1_packed: workspace =
 * frmap_match_workspace_bytes(B, G) bytes, probe_split = B * 3 * D fp16 of scratch; `gallery` is still the fp32 matrix
 * (candidates are re-scored from it). */
size_t frmap_match_gallery_pack_bytes(int G, int D);
int frmap_match_pack_gallery(const float* gallery, void* packed_out, float* stat_w_out, int G, int D, void* stream);
/* Incremental enrolment (src/app.py:428-436 appends one identity and re-saves): rows [row_lo, row_hi) of a gallery that now
 * holds G rows were appended (row_hi == G) or edited in place; only their statistics and the 64-row tiles they touch are
 * re-packed.  packed_out / stat_w_out must be sized for the gallery's CAPACITY (>= G rows).  As in frmap_match_pack_gallery the
 * packer itself takes packed_out 2-byte aligned; the calls that read the pack need 16. */
int frmap_match_pack_gallery_rows(const float* gallery, void* packed_out, float* stat_w_out, int row_lo, int row_hi,
                                  int G, int D, void* stream);
int frmap_match_top1_packed(const float* emb, const float* gallery, const void* gallery_packed, const float* stat_w,
                            int32_t* idx_out, float* dist_out, int32_t* id_or_unknown_out, int32_t* packed_out,
                            float thresh, void* workspace, void* probe_split, int B, int G, int D, void* stream);

/* Exact top-k gallery search: for each probe the k nearest gallery rows (entry mode, labels == NULL) or identities
 * (identity mode, labels = int32[G] >= 0: an identity's distance is the min over its rows, its representative the FIRST row
 * attaining that min) under the exact distance of frmap_match_top1: elements (e_i - g_i) + 1e-6 in fp32, squares summed in
 * float64, dist = (float)sqrt.  Ordered by (distance, row) ascending (ties go to the lower row, as in the reference loop).
 *   idx_out int32[B][k], dist_out fp32[B][k], label_out (optional) int32[B][k] (the label in identity mode, -1 in entry mode).
 *   Rows whose distance is NaN or +inf are never listed; positions past the last listable row / identity are
 *   (idx -1, dist +inf, label -1), which covers k > G and G == 0.  1 <= k <= 64, D % 4 == 0.
 *   k == 1 in entry mode runs frmap_match_top1 / frmap_match_top1_packed: bit-identical idx and dist.
 *   frmap_match_topk scans every row exactly (one wave per probe): for small galleries, or galleries without a pack.
 *   frmap_match_topk_packed: a gallery prepared by frmap_match_pack_gallery[_rows] (D % 32 == 0, G > 0) on the fp16 MFMA GEMM,
 *   whose epilogue keeps per probe and 64-row slot the 4 smallest lower bounds (rows + upper bounds) and a bound on the rest of
 *   the slot; every row that could be among the k nearest within the rounding bound is re-scored exactly.
 *   workspace: frmap_match_topk_workspace_bytes(B, G, D, k) bytes (records + statistics + the probes' fp16 split; device,
 *   caller-owned, 256-byte aligned).  Nothing is allocated or synchronised; every launch goes to `stream` (graph-capturable).
 *   Bad k, shape or pointer arguments are rejected before any launch. */
size_t frmap_match_topk_workspace_bytes(int B, int G, int D, int k);
int frmap_match_topk(const float* emb, const float* gallery, const int32_t* labels, int32_t* idx_out, float* dist_out,
                     int32_t* label_out, void* workspace, int B, int G, int D, int k, void* stream);
int frmap_match_topk_packed(const float* emb, const float* gallery, const void* gallery_packed, const float* stat_w,
                            const int32_t* labels, int32_t* idx_out, float* dist_out, int32_t* label_out,
                            void* workspace, int B, int G, int D, int k, void* stream);

/* Exact verification counts (the verification ROC of a set of labelled embeddings).  A = fp32 [P][D] with int32 labels [P],
 * B = fp32 [Q][D] with int32 labels [Q]; `thresholds` = fp32 [T] on the device, finite, >= 0 and strictly ascending,
 * 1 <= T <= 2048.  The distance of a pair is the one frmap_match_topk reports: dist(i, j) = (float) sqrt(d2), d2 = the squares of
 * the fp32 elements (a - b) + 1e-6 summed in float64.  A pair is accepted at t iff dist <= t (NaN / inf never), genuine iff
 * label_a[i] == label_b[j], impostor otherwise.  Counted pairs: a_row0 = -1 (cross mode): every (i, j); a_row0 >= 0 (self mode:
 * A is rows [a_row0, a_row0 + P) of B): the pairs with a_row0 + i < j, so a_row0 = 0 with A = B counts every unordered pair once
 * and shards over a_row0 sum to the whole.
 *   accepted_out: uint64 [2][T] = genuine / impostor pairs accepted at each t_k.  Exact integers, overwritten, independent of
 *                 path, tiling and launch order.  The totals follow from the label histograms.
 *   rescored_out: optional uint64 [1] = pairs re-scored exactly after the GEMM's error band straddled a threshold (0 on the scan).
 *   workspace:    frmap_verify_workspace_bytes(P, Q, D, T) bytes (device, caller-owned, 256-byte aligned).
 * frmap_verify_counts scores every counted pair exactly (small inputs, D % 32 != 0, B without a pack).
 * frmap_verify_counts_packed: B prepared by frmap_match_pack_gallery (D % 32 == 0, Q > 0) runs on the fp16 MFMA GEMM; its epilogue
 * bins every pair whose error band lies inside one threshold interval and re-scores the rest exactly.
 * Shapes, T, pointers and a_row0 are checked before any launch.  The threshold VALUES live on the device and are checked there
 * (nothing is synchronised, so the call can be graph-captured): a call whose thresholds break the contract writes all-ones
 * (UINT64_MAX) to every output. */
size_t frmap_verify_workspace_bytes(int P, int Q, int D, int T);
int frmap_verify_counts(const float* a, const int32_t* label_a, int P, const float* b, const int32_t* label_b, int Q, int D,
                        int a_row0, const float* thresholds, int T, uint64_t* accepted_out, uint64_t* rescored_out,
                        void* workspace, void* stream);
int frmap_verify_counts_packed(const float* a, const int32_t* label_a, int P, const float* b, const void* b_packed,
                               const float* stat_w, const int32_t* label_b, int Q, int D, int a_row0, const float* thresholds,
                               int T, uint64_t* accepted_out, uint64_t* rescored_out, void* workspace, void* stream);

/* Exact threshold search: WHICH pairs lie within a threshold (every enrolment a watch list should report for a probe, where
 * src/app.py:50-64 names only the nearest one; the duplicate pairs of a gallery that src/app.py:428-436 appends to without
 * de-duplicating; the impostor pairs behind a false-accept rate).  Operands, distance, a_row0 (cross / self mode, shards) as the
 * verification counts.  A counted pair (i, j) - i indexes A, j indexes B - is accepted iff dist(i, j) <= thresh (NaN / inf never)
 * and pair_filter lets it through: 0 = all pairs (labels may be NULL), 1 = equal labels only, 2 = different labels only.
 *   thresh:       finite, >= 0 (a host value: checked before any launch).
 *   count_out:    int32 [P]  = accepted pairs of row i of A;  total_out: uint64 [1] = accepted pairs.  Both exact whatever `capacity`.
 *   pair_out:     int32 [capacity][2] = (i, j);  dist_out: fp32 [capacity] = dist(i, j).  total <= capacity: slots [0, total) hold
 *                 every accepted pair exactly once, in no particular order; otherwise the first `capacity` slots hold distinct
 *                 accepted pairs.  capacity = 0 with NULL pair_out / dist_out is a count-only call.
 *   rescored_out: optional uint64 [1] = pairs the GEMM path scored exactly (0 on the scan).
 *   workspace:    frmap_match_radius_workspace_bytes(P, Q, D) bytes (device, caller-owned, 256-byte aligned).
 * frmap_match_radius scores every counted pair exactly.  frmap_match_radius_packed: B prepared by frmap_match_pack_gallery
 * (D % 32 == 0, Q > 0) runs on the fp16 MFMA GEMM, whose epilogue drops every pair whose error band lies beyond the threshold and
 * scores the rest exactly; a shape the GEMM does not take is answered as frmap_match_radius answers it.  Same outputs either way.
 * Nothing is allocated or synchronised; every launch goes to `stream` (graph-capturable).  Bad arguments are rejected (-1) before
 * any launch. */
size_t frmap_match_radius_workspace_bytes(int P, int Q, int D);
int frmap_match_radius(const float* a, const int32_t* label_a, int P, const float* b, const int32_t* label_b, int Q, int D,
                       int a_row0, float thresh, int pair_filter, int32_t* count_out, uint64_t* total_out, int32_t* pair_out,
                       float* dist_out, long long capacity, uint64_t* rescored_out, void* workspace, void* stream);
int frmap_match_radius_packed(const float* a, const int32_t* label_a, int P, const float* b, const void* b_packed,
                              const float* stat_w, const int32_t* label_b, int Q, int D, int a_row0, float thresh,
                              int pair_filter, int32_t* count_out, uint64_t* total_out, int32_t* pair_out, float* dist_out,
                              long long capacity, uint64_t* rescored_out, void* workspace, void* stream);

/* The tail of the ResNet-18 ('cnn') embed-and-match step for small galleries in ONE launch, one workgroup per face:
 * AdaptiveAvgPool2d(1) of the trunk map (face_models.py:100) -> optional F.normalize(eps) -> compare_faces' scan
 * (src/app.py:58-64): the first strict minimum, as frmap_match_top1 for G <= 64, but with the squares summed in fp32 (pooled 16-bit
 * maps are nowhere near the 2^64 at which an fp32 square overflows; a row whose fp32 sum does overflow is never the winner).
 *   map : [B][HW][C] (dtype) trunk output (NHWC);  gallery : fp32 [G][C], 0 <= G <= 64
 *   emb_out : fp32 [B][C] pooled (and normalised, if asked) embedding, or NULL;  other outputs as frmap_match_top1.
 * A face whose map holds a NaN / inf gets the NaN / inf embedding F.normalize would give (a NaN norm makes the row NaN) and is
 * declined: idx -1, dist +inf, id -1.  Other faces keep their answers bit for bit. */
int frmap_gap_norm_match(const void* map, const float* gallery, float* emb_out, int32_t* idx_out, float* dist_out,
                         int32_t* id_or_unknown_out, int32_t* packed_out, float thresh, int normalize, float eps,
                         int B, int HW, int C, int G, int dtype, void* stream);
/* Pool + Linear + normalise heads in one launch: AdaptiveAvgPool2d(1) of the NHWC trunk map [B][HW][K] -> Linear(K, N)
 * (y * scale + shift: a folded BatchNorm1d, or scale = NULL and shift = the bias) -> optional ReLU -> F.normalize(eps).
 *   ArcFaceNet (src/face_models.py:573-590): embedding (no bias) + bn, relu = 0;
 *   BaselineNet (:41-46, 51-60): F.relu(self.fc1(pooled)), relu = 1 (pre_out = the reference's un-normalised embedding).
 * wt: the Linear weight transposed, fp32 [K][N], N in {256, 512}; pre_out / emb_out: fp32 [B][N] un-normalised /
 * unit-norm embeddings (either may be NULL).  A NaN / inf in a face's map makes that face's pre_out / emb_out rows NaN / inf as in
 * PyTorch (the ReLU and the normalisation keep NaN); other faces keep their bits. */
int frmap_gap_linear_norm(const void* map, const float* wt, const float* scale, const float* shift, float* pre_out,
                          float* emb_out, float eps, int B, int HW, int K, int N, int relu, int dtype, void* stream);
int frmap_cosine_logits(const float* x, const float* w, float* logits_out, int32_t* argmax_out,
                        void* workspace, int B, int C, int D, float s, void* stream);
int frmap_arcmargin_eval(const float* x, const float* w, const int64_t* label, float* logits_out,
                         float* minmax_out, void* workspace, int B, int C, int D, float s, float m,
                         int easy_margin, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Model handles: what `model(images)` / `model.get_embedding(images)` run in the reference
 * (src/testing.py:255-273, src/app.py:44) as ONE call, for the ResNet-18 families of get_model()
 * (src/face_models.py:785-813): 'baseline' = BaselineNet (:16-60), 'cnn' = ResNetTransfer (:62-102), 'siamese' = SiameseNet
 * (one tower of forward(x1, x2), :104-192; 256-d embeddings), 'arcface' = ArcFaceNet eval (:447-613), 'hybrid' = HybridNet
 * (:650-721), 'resnet18_trunk' = the bare trunk (features only; AttentionNet builds on it, :269).
 *
 *   frmap_model_create       model_type as get_model() spells it; num_classes sizes the classifier head; `dtype` = compute type.
 *                            An unknown type is rejected with the reference's message ("Invalid model type: ...", :813).
 *   frmap_model_load_tensor  one call per entry of the reference checkpoint's state_dict, under the SAME key
 *                            ("resnet.layer1.0.bn1.running_var", "backbone.conv1.weight" or its alias "features.0.weight",
 *                            "embedding.weight", "bn.weight", "val_classifier.bias", ...): fp32 data, `numel` elements, host
 *                            memory (on_device = 0) or device memory (1).  Returns 0 = taken, 1 = a key the inference path does
 *                            not use (ignored: training head, num_batches_tracked), -1 = wrong size.
 *   frmap_model_finalize     folds every eval-mode BatchNorm into its conv / linear (fp32), packs the weights into the kernels'
 *                            layout, fixes the layer plan; fails naming the first missing tensor.  Synchronises `stream` once.
 *                            The fold is scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale (+ bias *
 *                            scale) with eps = 1e-5 ALWAYS: a state_dict does not carry eps, so a checkpoint of a module built with
 *                            another BatchNorm eps must be planned by the caller (the Python surface refuses such a module).
 *                            After it the handle is immutable: any thread / stream may run forwards on it concurrently.
 *   frmap_model_forward      x: FRMAP_INPUT_F32_NCHW = fp32 [B][3][H][W] (the reference's tensor) or FRMAP_INPUT_U8_HWC = uint8
 *                            [B][H][W][3] (ToTensor + Normalize applied inside the stem, src/testing.py:99-104);
 *                            `what` selects the output written to the caller-owned `out`:
 *                              FRMAP_OUT_TRUNK_MAP  [B][h][w][512] in `dtype`  (children()[:-2], face_models.py:660)
 *                              FRMAP_OUT_POOLED     fp32 [B][512]              (children()[:-1] flattened, :100,464)
 *                              FRMAP_OUT_EMBEDDING  fp32 [B][frmap_model_embedding_dim]: get_embedding() - 'cnn': the pooled features
 *                                                   (:98-102); 'arcface': F.normalize(bn(embedding(pooled))) (:584-590); 'baseline':
 *                                                   relu(fc1(pooled)) (:51-60); 'siamese': the tower's unit-norm output (:161-179);
 *                                                   'hybrid': LayerNorm(token mean) (:705-721)
 *                              FRMAP_OUT_LOGITS     fp32 [B][num_classes]: forward() - 'cnn': resnet.fc (:93-96); 'arcface':
 *                                                   val_classifier over row-normalised weights (:576-580); 'baseline': fc2;
 *                                                   'hybrid': fc; 'siamese': none (rejected)
 *                            (TRUNK_MAP / POOLED are the ResNet trunk's outputs: 'cnn', 'arcface', 'hybrid', 'resnet18_trunk'.)
 *                            workspace: frmap_model_workspace_bytes(m, B, H, W) bytes, 256-byte aligned, caller-owned.
 *                            x: 4-byte aligned for both input kinds - fp32: its element size, whatever the family and the size
 *                            (the stems and the layout kernel pick their wider paths from the pointer); uint8: where the fused
 *                            uint8 stem takes the image (W % 4 == 0 and a ResNet trunk up to ~224 wide or a siamese tower up to
 *                            ~256 wide); a uint8 image that goes through the byte-wise normalise kernel may start anywhere;
 *                            out: 16-byte aligned for FRMAP_OUT_TRUNK_MAP, 4 for the fp32 outputs.  The same x and workspace rules
 *                            hold for the two calls below, whose workspace is 256-byte aligned as well.
 *                            Nothing is allocated, freed or synchronised; all launches go to `stream`.
 *   frmap_model_embed_and_match  forward + compare_faces for every face (src/app.py:44,50-64): embedding (L2-normalised first if
 *                            `normalize`, for models whose embedding is not unit-norm) -> first arg-min of ||e - g + 1e-6||_2
 *                            over the fp32 gallery [G][512] -> outputs as frmap_match_top1.  gallery_packed / gallery_stat
 *                            (frmap_match_pack_gallery; may be NULL) put galleries of >= 512 rows on the MFMA pipe; 'cnn' with
 *                            G <= 64 pools, normalises and matches in one launch.  emb_out: optional fp32 [B][512].
 *                            workspace: frmap_model_match_workspace_bytes(m, B, H, W, G).
 *   frmap_model_embed_and_search  forward + exact top-k search (frmap_match_topk[_packed]): the embedding as
 *                            frmap_model_embed_and_match forms it (normalised if asked), then the k nearest rows (labels == NULL)
 *                            or identities (labels int32[G]) of the fp32 gallery [G][D]; outputs as frmap_match_topk.  k == 1 with
 *                            labels == NULL is frmap_model_embed_and_match (same idx and dist).  gallery_packed / gallery_stat
 *                            (may be NULL) put galleries of >= 512 rows on the MFMA pipe.  emb_out: optional fp32 [B][D].
 *                            workspace: frmap_model_search_workspace_bytes(m, B, H, W, G, k).
 *   frmap_model_trace / _trace_read  per-launch HIP-event timing of subsequent forwards (kernel label, algorithmic FLOPs and
 *                            bytes, microseconds) for roofline reports; read synchronises the recorded events and clears them.
 * ------------------------------------------------------------------------------------------- */
#define FRMAP_INPUT_F32_NCHW 0
#define FRMAP_INPUT_U8_HWC 1
#define FRMAP_OUT_TRUNK_MAP 0
#define FRMAP_OUT_POOLED 1
#define FRMAP_OUT_EMBEDDING 2
#define FRMAP_OUT_LOGITS 3
typedef struct frmap_model frmap_model;
typedef struct frmap_trace_record {
  char kernel[64];
  double flop;
  double bytes;
  float us;
} frmap_trace_record;
int frmap_model_create(frmap_model** out, const char* model_type, int num_classes, int dtype);
int frmap_model_load_tensor(frmap_model* m, const char* key, const void* data, size_t numel, int on_device);
int frmap_model_set_input_normalization(frmap_model* m, const float* mean3_host, const float* std3_host);
int frmap_model_finalize(frmap_model* m, void* stream);
int frmap_model_embedding_dim(const frmap_model* m);
size_t frmap_model_workspace_bytes(const frmap_model* m, int B, int H, int W);
size_t frmap_model_match_workspace_bytes(const frmap_model* m, int B, int H, int W, int G);
int frmap_model_forward(frmap_model* m, const void* x, int x_kind, int B, int H, int W, int what, void* out,
                        void* workspace, void* stream);
int frmap_model_embed_and_match(frmap_model* m, const void* x, int x_kind, int B, int H, int W, const float* gallery,
                                const void* gallery_packed, const float* gallery_stat, int G, float thresh, int normalize,
                                int32_t* idx_out, float* dist_out, int32_t* id_or_unknown_out, int32_t* packed_out,
                                float* emb_out, void* workspace, void* stream);
size_t frmap_model_search_workspace_bytes(const frmap_model* m, int B, int H, int W, int G, int k);
int frmap_model_embed_and_search(frmap_model* m, const void* x, int x_kind, int B, int H, int W, const float* gallery,
                                 const void* gallery_packed, const float* gallery_stat, const int32_t* labels, int G,
                                 int k, int normalize, int32_t* idx_out, float* dist_out, int32_t* label_out,
                                 float* emb_out, void* workspace, void* stream);
int frmap_model_trace(frmap_model* m, int enable);
int frmap_model_trace_read(frmap_model* m, frmap_trace_record* out, int max_records);
void frmap_model_destroy(frmap_model* m);

#ifdef __cplusplus
}
#endif
#endif /* FRMAP_HIP_H */
