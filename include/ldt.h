/*
 * ldt.h — C-ABI of libldt.so, the MI355X (gfx950) batch-decode path that
 * replaces lance-distributed-training's per-row PIL/torchvision transform.
 *
 * Drop-in boundary (reference = /root/reference, pure Python):
 *   - to_tensor_fn  decode_tensor_image(batch, **kwargs)   lance_iterable.py:38-50
 *       (registered at LanceDataset(..., to_tensor_fn=...) lance_iterable.py:53-59)
 *   - collate_fn    collate_fn(batch_of_dicts)             lance_map_style.py:21-44
 *       (registered at get_safe_loader(..., collate_fn=...) lance_map_style.py:60-69)
 *   - samplers      ShardedBatchSampler / ShardedFragmentSampler(pad=True)
 *                                                          lance_iterable.py:61-69
 * The reference has no FFI of its own (it is Python over pylance/Pillow); the
 * Python host package ldt_amd binds these symbols with ctypes, exactly as a
 * maintainer would (INTEGRATION.md shows the stub). No torch types cross this
 * boundary: plain pointers, sizes and an opaque hipStream_t passed as void*.
 *
 * Conventions
 *   - Every function returns an int status (LDT_OK == 0, negative = error);
 *     no C++ exception crosses the ABI. ldt_last_error() gives a message.
 *   - Host input pointers are borrowed for the duration of the call only: the
 *     call copies what it needs into the context's pinned staging ring before
 *     returning. Output device pointers are owned by the caller (torch).
 *   - Work is enqueued on `stream` (torch's current stream); results are
 *     stream-ordered. One context per (process, device); a context is not
 *     thread-safe.
 */
#ifndef LDT_H
#define LDT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (return values) ---- */
#define LDT_OK 0
#define LDT_ERR_ARG -1        /* bad argument                                  */
#define LDT_ERR_HIP -2        /* a HIP runtime call failed                     */
#define LDT_ERR_NOMEM -3      /* host/device allocation failed                 */
#define LDT_ERR_IMAGE -4      /* >= 1 image failed: see per_image_status       */

/* ---- per-image status codes (per_image_status[i]) ---- */
#define LDT_IMG_OK 0
#define LDT_IMG_NOT_JPEG 1    /* no SOI / malformed marker segments            */
#define LDT_IMG_UNSUPPORTED 2 /* arithmetic, lossless, 12-bit, CMYK, multi-scan sequential, a progressive file libjpeg would block-smooth, more than 10 blocks per MCU, a sampling factor that does not divide the largest, or subsampled luma (a chroma factor above luma's: libjpeg decodes such a file, this library does not) */
#define LDT_IMG_CORRUPT 3     /* entropy data truncated or restart markers wrong */
#define LDT_IMG_TOO_LARGE 4   /* dimension beyond LDT_MAX_DIM, or reduced by
                                 more than 37 on an axis: ceil(width / out_w) or
                                 ceil(height / out_h) > 37 (75 resize taps; at
                                 the default 224 x 224 that is LDT_MAX_DIM);
                                 with a crop (ldt_set_crops) the reduction is
                                 that of the row's box; with a window
                                 (ldt_set_windows) it is that of the box (or
                                 the whole image) against the resized size:
                                 ceil(src_w / res_w) or ceil(src_h / res_h) > 37;
                                 under LDT_FILTER_BICUBIC (ldt_set_filter) the
                                 filter's support of 2 doubles the taps, so
                                 every one of these limits is
                                 ceil(2 * src / res) > 37 (at 224 x 224:
                                 sources beyond 4144 px)                       */
#define LDT_IMG_NULL 5        /* null cell                                     */
#define LDT_IMG_BAD_CROP 6    /* the row's crop (ldt_set_crops): an empty box, a
                                 negative origin, a box not inside the decoded
                                 image, or flip not 0 or 1                     */
#define LDT_IMG_BAD_WINDOW 7  /* the row's window (ldt_set_windows): res_h or
                                 res_w outside 1..LDT_MAX_RES, a negative top or
                                 left, or an out_h x out_w window at (top, left)
                                 that is not inside res_h x res_w (nothing is
                                 padded)                                       */

#define LDT_MAX_DIM 8192      /* max width/height of a file's image (drafted or not: ldt_set_draft) */
#define LDT_MAX_OUT 1024      /* max output height/width (ldt_set_output_size) */
#define LDT_MAX_VIEWS 16      /* max views per image of a decode call (ldt_set_views) */
#define LDT_MAX_RES 65535     /* max resized height/width of a window row
                                 (ldt_set_windows)                             */

/* ---- options (ldt_set_option) ---- */
#define LDT_OPT_SYNC_STATUS 1 /* 1 (default): decode calls wait for the stream and
                                 report device-side per-image errors before
                                 returning; 0: asynchronous, errors are read
                                 later with ldt_fetch_status()                  */
#define LDT_OPT_HUFF_MODE 2   /* 0 auto (default) and 2: the parallel
                                 self-synchronising decoder, one workgroup per
                                 image (the serial one for images with > 256
                                 restart segments); 1: serial per segment      */
#define LDT_OPT_SUBSEQ_BITS 3 /* minimum subsequence length of the parallel
                                 decoder: 64..8192 bits, multiple of 32
                                 (default 256); each image uses the smallest
                                 S >= this that fits its slots in 1024 lanes   */
#define LDT_OPT_PROFILE 4     /* 1: record HIP events around every stage on the
                                 caller's stream (read with ldt_stage_times)    */
#define LDT_OPT_RESIZE_IMPL 5 /* 0 auto (default): one wave per band
                                 (k_resize4), the streaming workgroup kernel for
                                 sources wider than 1120 px, 4:2:0 sources
                                 <= 512 px wide with the fancy upsampling on
                                 packed 16-bit pairs (k_resize4<5>); 1: the
                                 same with 32-bit upsampling (k_resize4<0>,
                                 round 3's default, cross-check); 2: the
                                 streaming kernel for all (cross-check); 3: as
                                 0 with the generic-width band kernel (the one
                                 every output size but 224 x 224 takes) at
                                 224 x 224 too (cross-check, measuring aid).
                                 Output sizes wider than 256, batches with
                                 crops or windows and batches whose filter is
                                 not bilinear (ldt_set_filter) take the
                                 streaming kernel under every value            */
#define LDT_OPT_SYNC_WARM 7   /* parallel decoder phase 1 starts this % of S
                                 before each range (0..200, default 0)         */
#define LDT_OPT_COPY_THREADS 8 /* threads of the context's host copy pool that
                                 move a batch's cells into the pinned slot while
                                 the calling thread walks the headers (0..31;
                                 -1 = default: the cgroup CPU quota divided by
                                 LOCAL_WORLD_SIZE, minus 2, at most 6)         */
#define LDT_OPT_HOST_TIMING 9 /* 1: accumulate host phase times of every
                                 decode call (read with ldt_host_times)        */
#define LDT_OPT_RESIZE_WAVES_PCT 10 /* resize bands per batch as % of one full
                                 wave of resize waves on the device (10..1000,
                                 default 100); more bands fill the pipeline's
                                 CU gaps, fewer keep the kernel efficient      */
#define LDT_OPT_DEBUG_COUNTERS 16 /* 1: the decoders count their phases (cycle
                                 stamps, rounds, symbols) into the plan blob,
                                 read with ldt_debug_counters; 0 (default): no
                                 counters (their atomics cost kernel time)     */
#define LDT_OPT_HUFF_WINDOW 17 /* cap in bytes on the parallel Huffman decoder's
                                 LDS stream window (-1, the default: what the
                                 CU's LDS leaves; 0: every stream read from
                                 global memory, destuffed by k_destuff_*) --
                                 a study knob                  */
#define LDT_OPT_RESIZE_WG_WAVES 15 /* waves (one band each) per k_resize4
                                 workgroup for JPEG sources: 0 default (4),
                                 1, 2 or 4 (tuning knob: 4 keeps 12 waves
                                 per CU at 512 px)           */
#define LDT_OPT_FUSED_DESTUFF 11 /* 1 (default): the parallel Huffman decoder
                                 destuffs the scan bytes of an image whose
                                 stream fits its LDS window itself; 0: every
                                 image through the k_destuff_* kernels
                                 (cross-check)                                  */
#define LDT_OPT_COPY_MODE 12  /* 0 (default): a host batch's cells go to HBM in
                                 one DMA on a per-device copy stream, which
                                 `stream` waits for (the transfer overlaps the
                                 kernels of earlier batches); 1: the DMA on
                                 `stream` itself                              */
#define LDT_OPT_COPY_BIND 13  /* 2 (default): copy-pool threads placed on
                                 physical cores local to the GPU's NUMA node,
                                 spread over its L3 domains, the block of
                                 cores chosen by LOCAL_RANK, each thread free
                                 to run on any CPU of its core's L3 domain;
                                 1: each thread pinned to its core; 0: unbound */
#define LDT_OPT_COPY_NT 14    /* 1 (default): the copy pool writes the pinned slot with
                                 non-temporal stores (AVX2, default); 0: memcpy */
#define LDT_OPT_SYNC_CACHE 19  /* the parallel Huffman decoder's table of converged
                                 slot states: 1 (default) a cell
                                 decoded before skips phase 1 and the rounds, on
                                 hints its write pass verifies; 2: the same and
                                 the kernel counts into ldt_sync_cache_stats
                                 (one atomic per image); 0: off, nothing is
                                 looked up, inserted or allocated. Bypassed
                                 while LDT_OPT_DEBUG_COUNTERS = 1.             */
#define LDT_OPT_SYNC_CACHE_MB 20 /* payload budget of the device's table in MiB
                                 (0..65536, default 1024: 131,072 entries of
                                 8 KiB; headers add 0.2%). One table per
                                 device, shared by the process's contexts,
                                 allocated by the first decode that uses it.
                                 A change frees the table (and its entries);
                                 make it while no other thread decodes on the
                                 device.                                       */

/* ---- stages reported by ldt_stage_times ---- */
#define LDT_OPT_VIEW_ORDER 18 /* grid order of k_resize_views (calls with
                               * ldt_set_views > 1 only). 0 (default): the
                               * views of an image follow each other in launch
                               * order; 1: view-major launch order. Both keep an
                               * image's workgroups on one blockIdx % 8. The
                               * output does not depend on it (A/B). */
#define LDT_STAGE_H2D 0       /* cell + plan copies into HBM                   */
#define LDT_STAGE_DESTUFF 1   /* coefficient clear + k_destuff                 */
#define LDT_STAGE_HUFFMAN 2   /* k_huff_*                                      */
#define LDT_STAGE_IDCT 3      /* k_idct, or k_idct_scaled (ldt_set_draft)      */
#define LDT_STAGE_RESIZE 4    /* k_resize (fused upsample/colour/resize/store) */
#define LDT_STAGE_COLOR 5     /* k_color_mean + k_color_apply + k_color_blur, the
                                 augment kernels, k_mix_apply + k_mix_labels (calls
                                 with ldt_set_colors, ldt_set_augments or ldt_set_mix
                                 only; never recorded otherwise) */
#define LDT_NUM_STAGES 6

typedef struct ldt_ctx ldt_ctx;

/* Normalize(mean, std) applied after ToTensor (lance_iterable.py:31). */
typedef struct {
  float mean[3];
  float std[3];
} ldt_norm;

/* Create a decode context on HIP device `device`. max_batch_bytes / max_n are
 * initial workspace hints (buffers grow on demand). Returns NULL on failure. */
ldt_ctx *ldt_create(int device, size_t max_batch_bytes, int max_n);
void ldt_destroy(ldt_ctx *ctx);
const char *ldt_last_error(ldt_ctx *ctx);
int ldt_set_option(ldt_ctx *ctx, int option, int64_t value);
/* The hipStream_t a host batch's cells go to HBM on under LDT_OPT_COPY_MODE 0
 * (NULL, the default: a per-device copy stream the library creates). The
 * stream must outlive the context's use of it; the decode stream waits for
 * the DMA with an event, and the DMA waits for the slot's previous readers. */
int ldt_set_copy_stream(ldt_ctx *ctx, void *stream);
/* Library version string, e.g. "ldt 0.1.0 gfx950". */
const char *ldt_version(void);

/* Output size of the resize, torchvision's Resize((out_h, out_w)): each in
 * 1..LDT_MAX_OUT, else LDT_ERR_ARG. Context state, 224 x 224 until set; every
 * decode / resize call made afterwards reads out_img_dev as float32
 * [n, 3, out_h, out_w]. Calls are stream-ordered and carry the size they were
 * made with, so a change never disturbs a batch still in flight. A source
 * reduced by more than 37 on an axis fails (LDT_IMG_TOO_LARGE for a JPEG row,
 * LDT_ERR_ARG from ldt_resize_raw). ldt_get_output_size reads the size back
 * (either pointer may be NULL). */
int ldt_set_output_size(ldt_ctx *ctx, int out_h, int out_w);
int ldt_get_output_size(ldt_ctx *ctx, int *out_h, int *out_w);

/* The resize's filter, torchvision's interpolation= / Pillow's resample=:
 * LDT_FILTER_BILINEAR (Image.BILINEAR) or LDT_FILTER_BICUBIC (Image.BICUBIC,
 * a = -0.5), each bit-exact with Pillow's two-pass resize, uint8 image between
 * the passes included; any other value is LDT_ERR_ARG and changes nothing.
 * Context state like the output size: bilinear until set, sticky across calls,
 * and every decode / resize call carries the filter it was made with, so a
 * change never disturbs a batch in flight. It composes with crops, windows,
 * flip and Normalize unchanged. A BICUBIC batch always takes the streaming
 * resize kernel, and its reduction limit is ceil(2 * src / res) > 37 on an
 * axis (LDT_IMG_TOO_LARGE; LDT_ERR_ARG from ldt_resize_raw), src and res as
 * for LDT_IMG_TOO_LARGE above. ldt_get_filter reads it back. */
#define LDT_FILTER_BILINEAR 0
#define LDT_FILTER_BICUBIC 1
int ldt_set_filter(ldt_ctx *ctx, int filter);
int ldt_get_filter(ldt_ctx *ctx, int *filter);

/* The output's element type and layout: what the last stage of every resize
 * stores. LDT_DTYPE_F32 (the default), LDT_DTYPE_F16 and LDT_DTYPE_BF16 hold
 * ToTensor [+ Normalize]'s float32 value in that type, rounded to nearest even
 * exactly as torch's Tensor.to(dtype) rounds it (fp16 overflow is +-inf, fp16
 * subnormals are kept); LDT_DTYPE_U8 holds the Pillow-exact resized byte
 * itself, the image before ToTensor, and refuses a Normalize: a decode /
 * resize call with norm_or_null != NULL is then LDT_ERR_ARG with nothing
 * enqueued. LDT_LAYOUT_NCHW (the default) is [n, 3, out_h, out_w] contiguous;
 * LDT_LAYOUT_NHWC stores the same values as [n, out_h, out_w, 3] contiguous,
 * torch's channels_last: element (i, c, y, x) at ((i * out_h + y) * out_w + x)
 * * 3 + c. Context state with the rules of ldt_set_filter: F32 / NCHW until
 * set, sticky across calls, a bad value is LDT_ERR_ARG and changes nothing,
 * and every decode / resize call carries the format it was made with, so a
 * change never disturbs a batch in flight. The calls' signatures do not
 * change: out_img_dev keeps its declared type and is the base of
 * n * 3 * out_h * out_w elements of the format in force, aligned to the
 * element only. A failed row is all-zero bytes in every format. It composes
 * with sizes, crops, windows, flip, the filters and Normalize unchanged.
 * ldt_get_output_format reads it back (either pointer may be NULL). */
#define LDT_DTYPE_F32 0
#define LDT_DTYPE_F16 1
#define LDT_DTYPE_BF16 2
#define LDT_DTYPE_U8 3
#define LDT_LAYOUT_NCHW 0
#define LDT_LAYOUT_NHWC 1
int ldt_set_output_format(ldt_ctx *ctx, int dtype, int layout);
int ldt_get_output_format(ldt_ctx *ctx, int *dtype, int *layout);

/* Per-image crop box and horizontal flip: torchvision's
 * F.resized_crop(img, top, left, height, width, size) followed by hflip when
 * flip == 1 (RandomResizedCrop + RandomHorizontalFlip with the parameters
 * drawn by the caller). The box is taken from the fully decoded RGB image
 * (chroma upsampling still sees the neighbours outside it); the resize then
 * treats the box as the whole source (Pillow's crop().resize()), and output
 * column x of a flipped row lands at out_w - 1 - x. */
typedef struct {
  int32_t top, left, height, width, flip;
} ldt_crop;

/* Crops of the next decode or ldt_resize_raw call of the context, one per row
 * (host memory, copied during the call). That call consumes them, even when
 * it fails, and must have exactly n rows, else it returns LDT_ERR_ARG and
 * enqueues nothing. crops == NULL clears pending crops. A row whose box is
 * bad fails alone with LDT_IMG_BAD_CROP (ldt_resize_raw: LDT_ERR_ARG); the
 * reduction limit (LDT_IMG_TOO_LARGE) applies to the box: ceil(width / out_w)
 * or ceil(height / out_h) > 37 (LDT_FILTER_BICUBIC: ceil(2 * width / out_w) or
 * ceil(2 * height / out_h) > 37). With no crops pending every call behaves as
 * if this function did not exist. */
int ldt_set_crops(ldt_ctx *ctx, const ldt_crop *crops, int64_t n);

/* Per-image resized size and window: the row's source (its crop box when
 * crops are pending too, else the whole decoded image) is resized to
 * res_h x res_w, and the output is the out_h x out_w window
 * (ldt_set_output_size) of that result whose first pixel is (top, left):
 * Pillow's resize((res_w, res_h), BILINEAR).crop((left, top, left + out_w,
 * top + out_h)), bit for bit (BICUBIC under ldt_set_filter). torchvision's Resize(256) + CenterCrop(224) is
 * res = the shorter edge scaled to 256 and a centred 224 x 224 window. Only
 * the window's pixels are computed, by the streaming kernel only; the whole
 * image is still decoded. Order with crops: box -> resize -> window -> flip
 * (window column x of a flipped row lands at out_w - 1 - x). */
typedef struct {
  int32_t res_h, res_w, top, left;
} ldt_window;

/* Windows of the next decode or ldt_resize_raw call of the context, one per
 * row, with the lifetime of ldt_set_crops: host memory copied during the call,
 * consumed by that call even when it fails, exactly n rows or LDT_ERR_ARG with
 * nothing enqueued, windows == NULL clears. A row is bad when res_h or res_w
 * is outside 1..LDT_MAX_RES, top < 0, left < 0, out_h > res_h - top or
 * out_w > res_w - left: no padding, so where torchvision's CenterCrop would
 * pad, the row fails. A bad JPEG row fails alone with LDT_IMG_BAD_WINDOW
 * (ldt_resize_raw: LDT_ERR_ARG). The reduction limit (LDT_IMG_TOO_LARGE) is
 * that of the source against the resized size: ceil(src_w / res_w) or
 * ceil(src_h / res_h) > 37 (LDT_FILTER_BICUBIC: ceil(2 * src_w / res_w) or
 * ceil(2 * src_h / res_h) > 37). A row's window is checked before its box, so a
 * row with both bad reports LDT_IMG_BAD_WINDOW. With no windows pending every
 * call behaves as if this function did not exist. */
int ldt_set_windows(ldt_ctx *ctx, const ldt_window *windows, int64_t n);

/* Views per image of the next decode call of the context (1..LDT_MAX_VIEWS),
 * with the lifetime of ldt_set_crops: that call consumes the value even when
 * it fails, and 1 clears it. A value outside the range is LDT_ERR_ARG and
 * changes nothing. A call with views = V > 1 decodes each of its n cells once
 * and writes V * n images, view-major: out_img_dev is the base of
 * V * n * 3 * out_h * out_w elements and view v of row i is output image
 * v * n + i (element (v, i, c, y, x) of [V, n, 3, out_h, out_w]; under
 * LDT_LAYOUT_NHWC V * n HWC images), so each view is a dense batch. Pending
 * crops and windows then have n * V rows, image-major (row i, view v at
 * i * V + v), else LDT_ERR_ARG with nothing enqueued; a missing one means the
 * whole image without flip, or res = out and origin 0, for every view. Output
 * size, filter, format and Normalize are the call's and apply to every view.
 * per_image_status and the labels stay [n]: a row that fails to decode fails
 * all its views; otherwise its views are checked in order v = 0..V-1, each in
 * the order of a single view (window, crop, too large), and the first that
 * fails gives the row its code. A failed row is all-zero bytes in all V
 * outputs, label -100. Output image (v, i) is bit for bit what a single-view
 * call with row i's view-v crop and window gives. LDT_ERR_ARG as well when
 * V * n or the resize's workgroup count ((n rounded up to 8) * V * ceil(out_h
 * / 8) * ceil(out_w / 256)) does not fit an int. ldt_resize_raw with
 * views > 1 pending returns LDT_ERR_ARG and consumes it: a raw source has no
 * decode to share. With no views pending, or 1, every call behaves as if this
 * function did not exist. */
int ldt_set_views(ldt_ctx *ctx, int views);

/* One output size per view for the next decode call of the context: hw is
 * [views][2] as (h, w), each in 1..LDT_MAX_OUT, views in 1..LDT_MAX_VIEWS
 * (DINO / SwAV multi-crop: two views at 224 x 224 and six at 96 x 96 from one
 * decode). Pending like ldt_set_views: the next decode call consumes the sizes
 * even when it fails. A bad argument (count, range, NULL) is LDT_ERR_ARG and
 * changes nothing. The sizes imply views; ldt_set_views pending with another
 * count (other than 1) makes that call LDT_ERR_ARG with nothing enqueued, and
 * both are consumed. The context's own output size is not touched
 * (ldt_get_output_size reads the same before and after), and the next call
 * without sizes is a plain call.
 * Output behind out_img_dev, in elements of the call's dtype: the views dense
 * and back to back, view v starting at element n * 3 * sum over u < v of
 * h_u * w_u, image (v, i) i * 3 * h_v * w_v elements further on, each image
 * NCHW or NHWC dense; for equal sizes exactly ldt_set_views' [V, n, 3, h, w].
 * Crops and windows are those of ldt_set_views (n * V rows, image-major); view
 * v's window and reduction limit are checked against (h_v, w_v), and a missing
 * window is (h_v, w_v, 0, 0). Status, labels and failed rows are as for
 * ldt_set_views: the first view that fails gives the row its code, and the row
 * is zero bytes in all V outputs. views = 1 gives what a plain call at that
 * size gives. Output image (v, i) is bit for bit what a single-size call at
 * (h_v, w_v) with that view's crop and window gives. LDT_ERR_ARG as well when
 * the workgroup count ((n rounded up to 8) * sum over views of ceil(h_v / 8) *
 * ceil(w_v / 256)) does not fit an int. ldt_resize_raw with sizes pending
 * returns LDT_ERR_ARG and consumes them. */
int ldt_set_view_sizes(ldt_ctx *ctx, const int32_t *hw, int views);

/* The photometric stage of one output image: torchvision's
 * RandomApply([ColorJitter]), RandomGrayscale and RandomSolarize with the
 * parameters drawn by the caller, applied to the resized uint8 image exactly
 * as Pillow applies them (ImageEnhance.Brightness / Contrast / Color, the
 * convert("HSV") round trip of adjust_hue, convert("L"), ImageOps.solarize),
 * bit for bit, and Pillow's ImageFilter.GaussianBlur(radius) between the
 * grayscale and the solarize, bit for bit as well. 32 bytes.
 *   brightness, contrast, saturation : the factor, a float32 as Pillow's
 *                 (float)alpha; finite and >= 0; read only when its mask bit is set
 *   hue_shift   : 0..255, added to H modulo 256 (int(hue_factor * 255), wrapped)
 *   order[4]    : the permutation in which the four jitter ops are applied, op
 *                 codes 0 brightness, 1 contrast, 2 saturation, 3 hue
 *                 (torchvision's fn_idx); a permutation even when ops are absent
 *   mask        : bit k set = op k present (hue 0.0 is present: the HSV round
 *                 trip is lossy)
 *   gray        : 0 or 1
 *   solarize    : threshold 0..256, or -1 for none
 *   blur_ww, blur_r : the blur's weights as ldt_blur_weights gives them for
 *                 Pillow's radius; blur_ww == 0 = no blur (blur_r is then
 *                 ignored up to its range), so a record whose tail is zero
 *                 means what it meant before the blur existed. blur_r <= 7.
 *   pad_        : ignored */
typedef struct {
  float brightness, contrast, saturation;
  int32_t hue_shift;
  uint8_t order[4];
  uint8_t mask;
  uint8_t gray;
  int16_t solarize;
  uint32_t blur_ww;
  uint16_t blur_r;
  uint8_t pad_[2];
} ldt_color;

/* Colours of the next decode call of the context, with the lifetime of
 * ldt_set_crops: host memory copied by this call, consumed by the next decode
 * call even when it fails, colors == NULL clears. n_entries is n * views,
 * image-major like crops (row i, view v at i * V + v; n without views), else
 * that decode call returns LDT_ERR_ARG with nothing enqueued. An entry outside
 * the ranges above is LDT_ERR_ARG here and leaves nothing pending; so is one
 * with blur_r > 7, or with blur_ww != 0 and (2 * blur_r + 1) * blur_ww > 2^24
 * or (2 * blur_r + 3) * blur_ww < 2^24 (no pair ldt_blur_weights returns).
 * Stage order per output image: crop -> resize -> window -> flip, then the
 * jitter ops in `order`, then grayscale, then the blur, then solarize, then ToTensor /
 * Normalize and the store in the call's dtype and layout (under LDT_DTYPE_U8
 * the stored byte is the colour-processed byte). The contrast mean is
 * int(mean + 0.5) of L over that output image in the state it has when
 * contrast's turn comes. The resize runs as under LDT_DTYPE_U8 into a
 * workspace of the context; up to three more kernels (the mean, only when some
 * entry has contrast, the apply, and the blur, only when some entry has one:
 * it serves those entries, with all six passes in LDS) follow on the same
 * stream. A call whose entries have no blur launches what it launched before
 * the blur existed. A failed row stays
 * all-zero bytes. ldt_resize_raw with colours pending returns LDT_ERR_ARG and
 * consumes them: raw sources are out of scope. With no colours pending every
 * call behaves as if this function did not exist. */
int ldt_set_colors(ldt_ctx *ctx, const ldt_color *colors, int64_t n_entries);

/* Host only, no context, no HIP call: the weights of Pillow's
 * ImageFilter.GaussianBlur(radius) for ldt_color's blur_r and blur_ww. Pillow
 * blurs with three extended box blurs per axis; *r is the box's whole radius
 * and *ww the 24-bit fixed-point weight of each of its 2 * r + 1 taps, the two
 * taps beyond them weighing ((1 << 24) - (2 * r + 1) * ww) / 2. radius is
 * Pillow's, as a float32 (Pillow rounds it so), in [0, 8.0]: 8.0 gives r = 7,
 * the largest the kernel's halo takes; 0 gives (0, 1 << 24), the identity,
 * which a record states as blur_ww = 0. LDT_ERR_ARG for any other radius (NaN
 * included) or a NULL pointer. */
int ldt_blur_weights(float radius, int32_t *r, uint32_t *ww);

/* The auto-augment stage of one output image: up to LDT_MAX_AUG_OPS ops of the
 * op set of torchvision's TrivialAugmentWide / RandAugment / AutoAugment, with
 * the parameters drawn by the caller, applied in order to the resized uint8
 * image exactly as Pillow applies them to a PIL image, bit for bit, then an
 * optional erase box (RandomErasing(value=0) after Normalize). 192 bytes.
 *   count   : 0..LDT_MAX_AUG_OPS, the ops op[0..count) applied in that order
 *   erase   : (top, left, height, width) of the erase box in the output image;
 *             height == 0 = none (the other three are then ignored), else
 *             height >= 1, width >= 1 and the box inside the output image
 *             (checked by the decode call, which knows the size). Inside it
 *             the stored element is zero in every dtype
 *   op[k].code : LDT_AUG_*
 *     IDENTITY      nothing
 *     AFFINE        Image.transform(size, AFFINE, matrix, NEAREST, fillcolor):
 *                   a[6] are Pillow's 16.16 fixed-point coefficients of the
 *                   output -> input matrix m, a[k] = floor(v * 65536 + 0.5) of
 *                   v = m0, m1, m2 + m0 / 2 + m1 / 2, m3, m4, m5 + m3 / 2 +
 *                   m4 / 2; source pixel of (x, y): ((a2 + a0 x + a1 y) >> 16,
 *                   (a5 + a3 x + a4 y) >> 16), the fill outside the image. The
 *                   sums must stay inside int32 over the output image (checked
 *                   by the decode call: the one affine check the library makes).
 *                   Whether Pillow itself would take this walk for m is the
 *                   caller's to ensure, since the record no longer holds m:
 *                   Pillow walks in fixed point only when every corner (0, 0),
 *                   (w, 0), (0, h), (w, h) of the output maps inside +-32768
 *                   (|m0 x + m1 y + m2| and |m3 x + m4 y + m5| < 32768), and
 *                   sends a matrix with m1 == 0 and m3 == 0 through its scale
 *                   routine, which agrees with the walk for m0, m4 = +-1 and
 *                   integer m2, m5 (translations, flips) and not in general.
 *                   The Python validator (check_augments) refuses the rest
 *     BRIGHTNESS, COLOR, CONTRAST, SHARPNESS
 *                   ImageEnhance.*(image).enhance(factor); factor is Pillow's
 *                   (float)alpha, finite and >= 0
 *     POSTERIZE     ImageOps.posterize(image, param), param (bits) in 0..8
 *     SOLARIZE      v < param ? v : 255 - v, param (threshold) in 0..256
 *     AUTOCONTRAST  ImageOps.autocontrast(image)
 *     EQUALIZE      ImageOps.equalize(image)
 *     INVERT        255 - v
 *   fill, pad_ : the affine op's fill colour; ignored otherwise */
#define LDT_MAX_AUG_OPS 4
#define LDT_AUG_IDENTITY 0
#define LDT_AUG_AFFINE 1
#define LDT_AUG_BRIGHTNESS 2
#define LDT_AUG_COLOR 3
#define LDT_AUG_CONTRAST 4
#define LDT_AUG_SHARPNESS 5
#define LDT_AUG_POSTERIZE 6
#define LDT_AUG_SOLARIZE 7
#define LDT_AUG_AUTOCONTRAST 8
#define LDT_AUG_EQUALIZE 9
#define LDT_AUG_INVERT 10
typedef struct {
  int32_t code;
  int32_t param;
  float factor;
  uint8_t fill[3];
  uint8_t pad_;
  int32_t a[6];
} ldt_aug_op;
typedef struct {
  int32_t count;
  int32_t erase[4];
  int32_t pad_[3];
  ldt_aug_op op[LDT_MAX_AUG_OPS];
} ldt_aug;

/* Augments of the next decode call of the context, with the lifetime of
 * ldt_set_colors: host memory copied by this call, consumed by the next decode
 * call even when it fails, augs == NULL clears. n_entries is n * views,
 * image-major (row i, view v at i * V + v; n without views), else that decode
 * call returns LDT_ERR_ARG with nothing enqueued; so it does when an erase box
 * leaves its output image or an affine op's walk over its output image leaves
 * int32. An entry outside the ranges above is LDT_ERR_ARG here and leaves
 * nothing pending. Stage order per output image: crop -> resize -> window ->
 * flip, then the ops, then ToTensor / Normalize, the erase box and the store in
 * the call's dtype and layout. The resize runs as under LDT_DTYPE_U8 into a
 * workspace of the context; with K the largest count of the call, K slots
 * follow on the same stream (one when K is 0), each one launch of k_aug_apply,
 * preceded by one of k_aug_stats when some entry's op in that slot is CONTRAST,
 * AUTOCONTRAST or EQUALIZE. An entry with k ops runs them in the last k slots.
 * The stage is timed as LDT_STAGE_COLOR. A failed row stays all-zero bytes.
 * Augments and colours pending for the same call: LDT_ERR_ARG, nothing
 * enqueued, both consumed. ldt_resize_raw with augments pending returns
 * LDT_ERR_ARG and consumes them. With no augments pending every call behaves
 * as if this function did not exist. */
int ldt_set_augments(ldt_ctx *ctx, const ldt_aug *augs, int64_t n_entries);

/* The batch step of one row (MixUp / CutMix), fused as the last stage before
 * the store. Let x be the row's float32 value at an element (the ToTensor /
 * Normalize table's entry of its final byte, +0.0f inside its own erase box)
 * and p the same of row `partner` at the same element:
 *   inside the row's box : out = p
 *   elsewhere            : out = fl32(fl32(p * w_partner) + fl32(x * w_self))
 * both products rounded to float32 before the add (no FMA), no shortcut for
 * weights 0 or 1 nor for partner == the row itself. out is stored as float32,
 * or rounded to nearest even to fp16 (overflow to +-inf, subnormals kept) or
 * bf16: torch's .to(dtype) of the float32 result. With w_self = float32(lam),
 * w_partner = float32(1.0 - lam) that is torchvision v2's MixUp bit for bit;
 * CutMix is weights (1, 0) and a box.
 *   box : top, left, height, width in the output image; height == 0 = none
 * Soft labels (num_classes > 0), float32 [n][num_classes]: with a = the row's
 * label and b = its partner's, the row is zero except out[a] = lw_self and
 * out[b] = lw_partner when a != b, out[a] = fl32(lw_partner + lw_self) when
 * a == b. */
typedef struct {
  int32_t partner;
  float w_self, w_partner;
  int32_t box[4]; /* top, left, height, width; height == 0 = none */
  float lw_self, lw_partner;
  int32_t pad_;
} ldt_mix; /* 40 bytes */

/* The mix of the next decode call of the context, with the lifetime of
 * ldt_set_augments: host memory copied by this call, consumed by the next
 * decode call even when it fails, rows == NULL clears. LDT_ERR_ARG here, with
 * nothing left pending: a partner outside 0..n-1, a non-finite weight, a box
 * with height != 0 and height < 1, width < 1, top < 0 or left < 0,
 * num_classes outside 0..1<<20, num_classes > 0 with out_soft_dev == NULL.
 * LDT_ERR_ARG from the decode call, with nothing enqueued: n differs from the
 * batch, a box leaves the output size, views or a size list are pending as
 * well, the dtype is LDT_DTYPE_U8, num_classes > 0 and the call has no labels,
 * a row's label is outside 0..num_classes-1. Stage order per output element:
 * crop -> resize -> window -> flip -> colour ops or augment ops -> ToTensor /
 * Normalize -> erase box -> mix -> store. The call is staged as one with
 * colours or augments is; the colour or augment stage then writes uint8 planes
 * to a workspace and k_mix_apply reads a row's and its partner's planes, the
 * erase boxes from the ldt_aug records, and stores the call's output;
 * k_mix_labels (num_classes > 0 only) writes every element of out_soft_dev,
 * which the caller keeps alive like the call's other outputs. num_classes == 0
 * mixes images only and leaves out_soft_dev alone. The int64 labels are
 * written as before. Failed rows: all-zero bytes, an all-zero soft row, label
 * -100; a row whose partner failed is stored unmixed (its own x everywhere,
 * the box ignored), its soft row 1.0f at its label. Timed inside
 * LDT_STAGE_COLOR. ldt_resize_raw with a mix pending returns LDT_ERR_ARG and
 * consumes it. With no mix pending every call launches what it did before. */
int ldt_set_mix(ldt_ctx *ctx, const ldt_mix *rows, int64_t n, int32_t num_classes, float *out_soft_dev);

/* Draft scales of the next decode call of the context, one per row, each 1, 2,
 * 4 or 8, with the lifetime of ldt_set_crops: host memory copied by this call,
 * consumed by the next decode call even when it fails, scales == NULL clears.
 * A value outside {1, 2, 4, 8} is LDT_ERR_ARG here with nothing left pending;
 * an n that differs from the batch is LDT_ERR_ARG from the decode call with
 * nothing enqueued. A row with scale s decodes in the DCT domain to the
 * ceil(W / s) x ceil(H / s) image libjpeg gives at scale 1 / s, bit for bit
 * what Pillow's Image.draft("RGB", ...) and convert("RGB") give when draft
 * picks that scale: each block goes through libjpeg's reduced IDCT (4x4, 2x2,
 * 1x1; jidctred.c) of its component's DCT_scaled_size, subsampled chroma takes
 * the next larger IDCT instead of being upsampled, and at 1/8 fancy upsampling
 * is off (jdsample.c). These are NOT the pixels of the full decode resized:
 * the caller opts in. Everything downstream treats the drafted image as the
 * decoded image: crop boxes and windows are in its coordinates and checked
 * against its size (LDT_IMG_BAD_CROP, LDT_IMG_BAD_WINDOW), the reduction limit
 * of LDT_IMG_TOO_LARGE is that of the drafted source, views and size lists
 * share the one drafted decode, and filter, format, Normalize, colours,
 * augments and the mix compose unchanged. LDT_MAX_DIM stays a bound on the
 * file's own size, and ldt_image_sizes keeps reporting it. The Huffman stage
 * is unchanged (the whole stream is decoded); a batch with a drafted row runs
 * k_idct_scaled in place of k_idct, timed as LDT_STAGE_IDCT. ldt_resize_raw
 * with a draft pending returns LDT_ERR_ARG and consumes it. With no draft
 * pending, or all scales 1, every call launches what it did before. */
int ldt_set_draft(ldt_ctx *ctx, const int32_t *scales, int64_t n);

/* Host only, no context, no HIP call: width, height (wh[2 * i], wh[2 * i + 1])
 * and the LDT_IMG_* code the planner's marker walk gives each of the n cells
 * of an Arrow binary (offsets64 == 0: int32 offsets) or large_binary
 * (offsets64 != 0: int64) array, arguments as for ldt_decode_batch. A failed
 * row gets width and height 0. For sampling crop boxes before the decode.
 * Always the file's own size: a caller that drafts (ldt_set_draft) divides. */
int ldt_image_sizes(const uint8_t *data, const void *offsets, int offsets64, int64_t arr_offset,
                    int64_t n, const uint8_t *validity, int32_t *wh /* [n][2] */, int32_t *status);

/* decode_tensor_image / collate_fn core, Arrow `binary` column (int32 offsets).
 *   data, offsets      : the Arrow array's data and offsets buffers (host);
 *   arr_offset         : Array.offset (slices share buffers), in rows;
 *   n                  : rows;
 *   validity           : Arrow validity bitmap or NULL (a null cell -> LDT_IMG_NULL);
 *   labels             : int64 label buffer (host) or NULL, label_offset in rows;
 *   out_img_dev        : float32 [n, 3, out_h, out_w] contiguous, device
 *                        (ldt_set_output_size; [n, 3, 224, 224] by default);
 *                        under ldt_set_output_format the base of n * 3 * out_h
 *                        * out_w elements of the format in force; with
 *                        ldt_set_views = V pending, V times that, view-major;
 *   out_lbl_dev        : int64 [n], device (ignored when labels == NULL);
 *   norm_or_null       : NULL = ToTensor only, else Normalize(mean, std) fused;
 *   stream             : hipStream_t (void*), 0 = null stream;
 *   per_image_status   : int32 [n] host, written with LDT_IMG_* codes.
 * Replaces lance_iterable.py:41-49 (to_pylist + PIL open/convert + Resize +
 * ToTensor + stack) and lance_map_style.py:34-44. */
int ldt_decode_batch(ldt_ctx *ctx, const uint8_t *data, const int32_t *offsets,
                     int64_t arr_offset, int64_t n, const uint8_t *validity,
                     const int64_t *labels, int64_t label_offset, float *out_img_dev,
                     int64_t *out_lbl_dev, const ldt_norm *norm_or_null, void *stream,
                     int32_t *per_image_status);

/* Same, Arrow `large_binary` column (int64 offsets). */
int ldt_decode_batch_large(ldt_ctx *ctx, const uint8_t *data, const int64_t *offsets,
                           int64_t arr_offset, int64_t n, const uint8_t *validity,
                           const int64_t *labels, int64_t label_offset, float *out_img_dev,
                           int64_t *out_lbl_dev, const ldt_norm *norm_or_null, void *stream,
                           int32_t *per_image_status);

/* Device-resident input (bench / pre-staged loaders): the JPEG cells already
 * live in HBM at data_dev (same layout as the host copy data_host, which is
 * read only for the marker headers). offsets are int64, host, absolute byte
 * offsets of each cell in both buffers (n+1 entries). Labels as above. */
int ldt_decode_batch_resident(ldt_ctx *ctx, const uint8_t *data_host, const uint8_t *data_dev,
                              const int64_t *offsets, int64_t n, const int64_t *labels,
                              float *out_img_dev, int64_t *out_lbl_dev,
                              const ldt_norm *norm_or_null, void *stream,
                              int32_t *per_image_status);

/* Zero-copy host input. ldt_register_host page-locks [ptr, ptr+len) in place
 * (hipHostRegister) for every context of the process: a later ldt_decode_batch
 * whose cells lie inside a registered range copies them to HBM by DMA straight
 * from those pages, without the memcpy into the context's pinned ring. Meant
 * for a memory-mapped Arrow IPC / Lance fragment registered once (the
 * dataset's `image` data buffer), replacing the per-batch copy SURVEY.md
 * §8f row 1 names. The range must stay mapped until ldt_unregister_host(ptr),
 * which waits for the device first. Returns LDT_OK or LDT_ERR_* (a range the
 * driver cannot lock stays on the copying path). */
int ldt_register_host(ldt_ctx *ctx, const void *ptr, size_t len);
int ldt_unregister_host(ldt_ctx *ctx, const void *ptr);

/* Wait for the last decode on `stream` and merge device-side per-image errors
 * into per_image_status[n] (for LDT_OPT_SYNC_STATUS = 0). */
int ldt_fetch_status(ldt_ctx *ctx, void *stream, int32_t *per_image_status, int64_t n);

/* Tickets (LDT_OPT_SYNC_STATUS = 0): every decode call that enqueues work gets
 * the next ticket of its context (1, 2, ...; ldt_last_ticket returns the most
 * recent one, 0 before any). A context holds the device-side status of its
 * last two calls: ldt_fetch_status_ticket waits only for that call's batch
 * (not for newer work on the stream) and merges its errors as above; a ticket
 * older than the last two returns LDT_ERR_ARG. This lets a pipeline check a
 * batch two uses of the context later, long after it completed, instead of
 * synchronising on the batch just before it. Replaces the per-batch status
 * check of lance_iterable.py:42 (PIL raising in the loop) without a stall. */
int64_t ldt_last_ticket(ldt_ctx *ctx);
int ldt_fetch_status_ticket(ldt_ctx *ctx, int64_t ticket, int32_t *per_image_status, int64_t n);

/* Profiling (LDT_OPT_PROFILE = 1): waits for every recorded stage event and
 * adds the elapsed milliseconds of each stage since the last reset into
 * ms_out[stage] and the number of timed launches into count_out[stage]
 * (arrays of LDT_NUM_STAGES). reset != 0 clears the accumulators after reading. */
int ldt_stage_times(ldt_ctx *ctx, double *ms_out, int64_t *count_out, int reset);

/* Host phase times (LDT_OPT_HOST_TIMING = 1), microseconds summed over the
 * timed calls since the last reset, into us_out[LDT_NUM_HOST_PHASES]:
 * pinned slot + copy start, header walk (overlaps the cell copy), plan blob,
 * cell copy join + H2D enqueue, kernel launches, status; then two copy-pool
 * diagnostics that overlap those: the pool's wake-up (copy start to the first
 * chunk a pool thread took) and the copy's span (start to last chunk done);
 * *calls_out = calls. */
#define LDT_NUM_HOST_PHASES 8
int ldt_host_times(ldt_ctx *ctx, double *us_out, int64_t *calls_out, int reset);

/* The context's host copy placement as a JSON object (NUL-terminated, into
 * buf[len]): copy_threads, copy_cpus, gpu_numa (the GPU's NUMA node from
 * sysfs), quota_cpus (cgroup), local_rank / local_world (torchrun's
 * LOCAL_RANK / LOCAL_WORLD_SIZE), l3_domains, candidate_cores, and the
 * copy_bind / copy_nt / copy_mode options, local_cpulist (the GPU's local
 * CPUs from sysfs, "" if unknown). Creates the pool if needed. */
int ldt_host_info(ldt_ctx *ctx, char *buf, size_t len);

/* Diagnostics (LDT_OPT_DEBUG_COUNTERS = 1): waits for `stream`, then copies the
 * parallel Huffman decoder's 16 int32 counters of the last batch into out16,
 * summed over its images: [1] images, [2] convergence rounds (sum), [3] rounds
 * (max), [4] memo adoptions, [5] write-pass symbols (sum over lanes), [6] the
 * symbols of each wave's slowest lane (sum), [8] setup, [9] phase 1, [10]
 * rounds, [11] block-count scan, [12] write pass (10 ns ticks), [13] needy
 * slots and [14] the waves they ran on (summed over rounds); [0], [7], [15]
 * unused. LDT_ERR_ARG when no batch was decoded with the option on. */
int ldt_debug_counters(ldt_ctx *ctx, int32_t *out16, void *stream);

/* The device's sync cache (LDT_OPT_SYNC_CACHE). All three wait for the device
 * (every stream of every context on it) first; call them while no other
 * thread decodes on the device.
 * ldt_sync_cache_stats: out8 = [0] hits, [1] misses, [2] inserts, [3] inserts
 * refused (set full; there is no eviction), [4] entries rejected by the
 * validation, [5] fallbacks (hints that failed the write pass's verification;
 * the image was redone by the full path in the same launch), counted by
 * decodes under LDT_OPT_SYNC_CACHE = 2 since the last clear; [6] the table's
 * capacity in entries, [7] its bytes on the device (0: not allocated).
 * ldt_sync_cache_clear: empties the table and zeroes the statistics.
 * ldt_sync_cache_corrupt: a test hook. Rewrites the payloads of the READY
 * entries and returns how many it changed (< 0: an LDT_ERR code). mode 1:
 * every entry gets another entry's payload (what a key collision looks
 * like); 2: every exit position + 1; 3: one block moved from a slot to its
 * successor in the same segment (sums preserved; entries without such a
 * pair are left alone); 4: an exit position past every segment, a coefficient
 * index of 255 and a block count no slot can reach. Whatever the table holds, decodes stay exact. */
int ldt_sync_cache_stats(ldt_ctx *ctx, int64_t *out8);
int ldt_sync_cache_clear(ldt_ctx *ctx);
int ldt_sync_cache_corrupt(ldt_ctx *ctx, int mode);

/* Config 5: raw uint8 HWC cells (no JPEG) -> Resize((out_h, out_w)) [+Normalize]
 * -> float32 [n,3,out_h,out_w] (ldt_set_output_size; 224 x 224 by default).
 * `hwc` is a device pointer when hwc_is_device != 0,
 * else host (copied through the pinned ring). Cell i starts at
 * hwc + i * cell_stride bytes and is h*w*3 bytes. */
int ldt_resize_raw(ldt_ctx *ctx, const uint8_t *hwc, int hwc_is_device, int64_t n, int h, int w,
                   int64_t cell_stride, float *out_img_dev, const ldt_norm *norm_or_null,
                   void *stream);

/* ShardedBatchSampler index computation (README.md:257-271), on device.
 * Writes the rank's batch row ranges as int64 pairs [start, end) into
 * out_ranges_dev (capacity pairs) and the pair count into *out_count_dev.
 * Batch k = [k*B, min(k*B+B, num_rows)), rank r gets k = r, r+W, ... */
int ldt_shard_ranges(ldt_ctx *ctx, int64_t num_rows, int64_t batch_size, int rank,
                     int world_size, int64_t *out_ranges_dev, int64_t capacity,
                     int64_t *out_count_dev, void *stream);

/* ShardedFragmentSampler index computation (README.md:140-155), on device.
 * fragment_rows_dev: int64 [nfrag] rows per fragment (dataset order).
 * Writes records of 5 int64 {fragment, start, end, global_start, is_pad} for
 * the rank's batches (fragments r, r+W, ...; batches never cross fragments)
 * into out_dev (capacity records), and the record count into *out_count_dev.
 * pad_to < 0: no padding. pad_to >= 0: pad the rank's list to pad_to records
 * (the max-over-ranks count agreed by all_reduce(MAX)) with this build's rule:
 * cycle the rank's own batches; a rank with no rows cycles the global batch
 * list from index `rank`. *out_local_count_dev receives the unpadded count. */
int ldt_shard_fragments(ldt_ctx *ctx, const int64_t *fragment_rows_dev, int nfrag,
                        int64_t batch_size, int rank, int world_size, int64_t pad_to,
                        int64_t *out_dev, int64_t capacity, int64_t *out_count_dev,
                        int64_t *out_local_count_dev, void *stream);

/* torch.utils.data.DistributedSampler index computation, on device — the
 * map-style loader's sampler (lance_map_style.py:58 -> torch 2.10
 * torch/utils/data/distributed.py:94-103 (num_samples) and :107-141 (__iter__)).
 * Writes the rank's num_samples indices (int64) into out_dev (capacity
 * entries) and num_samples into *num_samples_out (host, may be NULL):
 *   perm = torch.randperm(dataset_len, generator=manual_seed(seed)) when
 *   shuffle != 0 (bit-exact: MT19937 seeded with the low 32 bits of the 64-bit
 *   torch seed, forward Fisher-Yates), else the identity; padded by wrapping
 *   (drop_last == 0) or truncated; then every num_replicas-th from rank.
 * `seed` is the sampler's seed + epoch as torch's uint64 seed (two's complement
 * for negative values). dataset_len must be < 2^32/20 (torch draws 64-bit
 * numbers beyond that). */
int ldt_distributed_indices(ldt_ctx *ctx, int64_t dataset_len, int num_replicas, int rank,
                            int shuffle, uint64_t seed, int drop_last, int64_t *out_dev,
                            int64_t capacity, int64_t *num_samples_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LDT_H */
