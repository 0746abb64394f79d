/* h264mi -- MI355X-native H.264 Baseline macroblock-reconstruction engine.
 *
 * C-ABI of libh264mi.so (plain pointers and sizes only).  Three layers:
 *
 * 1. The Broadway decoder API (drop-in for Decoder/inc/H264SwDecApi.h):
 *    H264SwDecInit / Decode / NextPicture / GetInfo / Release /
 *    GetAPIVersion with the same structures, return codes and call
 *    protocol.  Replaces reference H264SwDecApi.c:124-569.
 * 2. The wasm/JS glue API (drop-in for Decoder/src/Decoder.c:44-185):
 *    broadwayInit / broadwayCreateStream / broadwayPlayStream / broadwayExit /
 *    broadwayGetMajorVersion / broadwayGetMinorVersion, calling back into
 *    broadwayOnHeadersDecoded / broadwayOnPictureDecoded, which the embedder
 *    registers with broadwaySetCallbacks (the emscripten library.js:1-13
 *    bridge becomes a function-pointer registration).
 * 3. The batched engine API used for multi-stream throughput (one picture
 *    from each of S streams per launch): h264mi_engine_*.
 *    This is the hot path the reference has no equivalent for; its unit of
 *    work is the MB-record batch of include/h264mi_records.h.
 */
#ifndef H264MI_H
#define H264MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------- */
/* 1. H264SwDec API  (reference Decoder/inc/H264SwDecApi.h:53-173)         */
/* ---------------------------------------------------------------------- */
typedef uint8_t  u8;
typedef uint32_t u32;
typedef int32_t  i32;

typedef enum {
    H264SWDEC_OK = 0,
    H264SWDEC_STRM_PROCESSED = 1,
    H264SWDEC_PIC_RDY,
    H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY,
    H264SWDEC_HDRS_RDY_BUFF_NOT_EMPTY,
    H264SWDEC_PARAM_ERR = -1,
    H264SWDEC_STRM_ERR = -2,
    H264SWDEC_NOT_INITIALIZED = -3,
    H264SWDEC_MEMFAIL = -4,
    H264SWDEC_INITFAIL = -5,
    H264SWDEC_HDRS_NOT_RDY = -6,
    H264SWDEC_EVALUATION_LIMIT_EXCEEDED = -7
} H264SwDecRet;

typedef void *H264SwDecInst;

typedef struct {
    u8  *pStream;
    u32  dataLen;
    u32  picId;
    u32  intraConcealmentMethod;
} H264SwDecInput;

typedef struct {
    u8  *pStrmCurrPos;
} H264SwDecOutput;

typedef struct {
    u32 *pOutputPicture;     /* planar I420, picWidth*picHeight*3/2 bytes */
    u32 picId;
    u32 isIdrPicture;
    u32 nbrOfErrMBs;
} H264SwDecPicture;

typedef struct {
    u32 cropLeftOffset;
    u32 cropOutWidth;
    u32 cropTopOffset;
    u32 cropOutHeight;
} CropParams;

typedef struct {
    u32 profile;
    u32 picWidth;            /* MB-aligned, pixels */
    u32 picHeight;
    u32 videoRange;
    u32 matrixCoefficients;
    u32 parWidth;
    u32 parHeight;
    u32 croppingFlag;
    CropParams cropParams;
} H264SwDecInfo;

typedef struct {
    u32 major;
    u32 minor;
} H264SwDecApiVersion;

H264SwDecRet H264SwDecInit(H264SwDecInst *decInst, u32 noOutputReordering);   /* H264SwDecApi.c:124 */
H264SwDecRet H264SwDecDecode(H264SwDecInst decInst, H264SwDecInput *pInput,
                             H264SwDecOutput *pOutput);                          /* :338 */
H264SwDecRet H264SwDecNextPicture(H264SwDecInst decInst, H264SwDecPicture *pOutput,
                                  u32 endOfStream);                              /* :524 */
H264SwDecRet H264SwDecGetInfo(H264SwDecInst decInst, H264SwDecInfo *pDecInfo);  /* :204 */
void H264SwDecRelease(H264SwDecInst decInst);                                    /* :259 */
H264SwDecApiVersion H264SwDecGetAPIVersion(void);

/* Application hooks (reference inc/H264SwDecApi.h:160-173).  The library
 * allocates / frees each instance through H264SwDecMalloc / H264SwDecFree
 * (H264SwDecApi.c:147, :301) and calls H264SwDecTrace with the API trace when
 * built with -DH264DEC_TRACE.  libh264mi.so carries the reference's default
 * definitions (malloc / free / memcpy / memset, H264SwDecApi.c:78-96); an
 * application defining its own (DecTestBench.c:678-760) overrides them. */
void  H264SwDecTrace(char *string);
void *H264SwDecMalloc(u32 size);
void  H264SwDecFree(void *ptr);
void  H264SwDecMemcpy(void *dest, void *src, u32 count);
void  H264SwDecMemset(void *ptr, i32 value, u32 count);                                /* :487 */
/* NextPicture, the picture converted to RGBA on the GPU: what Decoder.js
 * delivers with `rgb: true` (templates/DecoderPost.js:82-97, the asm.js
 * converter :322-560, per pixel yuv2rgbcalc :514-560).  rgba: picWidth *
 * picHeight * 4 bytes; pOutput->pOutputPicture = rgba.  No reference C
 * counterpart: the reference converts in JavaScript. */
H264SwDecRet H264SwDecNextPictureRGBA(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer, u8 *rgba);
/* NextPicture, the picture cropped to the active SPS's crop window on the GPU:
 * what DecTestBench -C writes (CropPicture, DecTestBench.c:588-666) and what
 * the player displays (YUVCanvas croppingParams).  dst receives cropOutWidth *
 * cropOutHeight * 3 / 2 bytes of I420, or with rgba != 0 cropOutWidth *
 * cropOutHeight * 4 bytes of RGBA (H264SwDecGetInfo's cropParams; with
 * croppingFlag == 0 the whole picture, as NextPicture / NextPictureRGBA
 * deliver it); pOutput->pOutputPicture = dst.  H264SWDEC_PARAM_ERR when the
 * backend cannot crop: there is no host fallback. */
H264SwDecRet H264SwDecNextPictureCropped(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer, u8 *dst,
                                         u32 rgba);
/* A picture as a planar tensor in device memory (tensor.hip): the window (x, y,
 * cw, ch -- luma pixels, all even) as (3, ch, cw) R G B planes (by default the
 * values of NextPictureRGBA; other colour sets below) or one (1, ch, cw) luma plane, contiguous, of uint8 (the
 * sample) or fp16 / bf16 / fp32: fma((float)sample, scale[p], bias[p]) of plane
 * p as one fp32 fused multiply-add, then rounded to nearest-even to the 16-bit
 * types.  GRAY uses scale[0] and bias[0]; uint8 ignores both. */
enum { H264MI_TENSOR_RGB = 0, H264MI_TENSOR_GRAY = 1 };
enum { H264MI_TENSOR_U8 = 0, H264MI_TENSOR_F16 = 1, H264MI_TENSOR_BF16 = 2, H264MI_TENSOR_F32 = 3,
       H264MI_TENSOR_I16 = 4 };     /* int16: the MB side-information field below only */
typedef struct { int x, y, cw, ch, mode, dtype; float scale[3], bias[3]; } h264mi_tensor_desc;
/* The colour set of an RGB tensor travels in `mode`: bits 0..7
 * the layout above, bits 8..11 the colour id, bits 12..13 (read only with
 * H264MI_TENSOR_COLOUR_STREAM) the set family to take where the stream names
 * none; every other bit zero, and bits 8..13 zero with GRAY.  A set is six
 * integers (ky, k0, crv, cgu, cgv, cbu); with u = U - 128, v = V - 128:
 *   a0 = ky Y + k0
 *   R = clamp((a0 + crv v) >> 10, 0, 255)
 *   G = clamp((a0 - cgu u - cgv v) >> 10, 0, 255)
 *   B = clamp((a0 + cbu u) >> 10, 0, 255)               (arithmetic shifts)
 *   id  set                              ky  yoff   crv  cgu  cgv   cbu
 *   0   reference (BT.601 limited,     1192   16   1634  400  832  2066
 *       DecoderPost.js; the default)
 *   1   BT.601 full range              1024    0   1436  352  731  1815
 *   2   BT.709 limited range           1192   16   1836  218  546  2163
 *   3   BT.709 full range              1024    0   1613  192  479  1900
 * Set 0 is NextPictureRGBA's converter, which does not round: k0 = -ky yoff.
 * Sets 1..3 round to nearest, k0 = 512 - ky yoff, and their coefficients are
 * floor(1024 c + 1/2) of c = 255/219 (ky, limited) and f 2 (1 - Kr), f 2 Kb
 * (1 - Kb) / Kg, f 2 Kr (1 - Kr) / Kg, f 2 (1 - Kb) with f = 255/224 (limited)
 * or 1 (full), (Kr, Kb) = (0.299, 0.114) or (0.2126, 0.0722), Kg = 1 - Kr - Kb.
 * Chroma is the 4:2:0 sample of the 2x2 block, replicated, as for set 0; the
 * values stay gamma-encoded R'G'B'.
 * H264MI_TENSOR_COLOUR_STREAM (the two H264SwDec calls below only; the engine-
 * level exports know no stream and refuse it) takes the set from the VUI of
 * the SPS the delivered picture was decoded under: matrix_coefficients 1 is
 * BT.709, 5 and 6 are BT.601; no VUI, no colour description, 2 (unspecified)
 * and every other value give the family of bits 12..13 -- BT.601, BT.709, or
 * by size: BT.709 when the export window (before any resize) is at least 1280
 * wide or more than 576 high.  The range is video_full_range_flag where the
 * VUI carries a video signal type, else limited.  With STREAM, BT.601 limited
 * range is set 0 (the reference's). */
enum { H264MI_TENSOR_COLOUR_REFERENCE = 0, H264MI_TENSOR_COLOUR_BT601_FULL = 1, H264MI_TENSOR_COLOUR_BT709 = 2,
       H264MI_TENSOR_COLOUR_BT709_FULL = 3, H264MI_TENSOR_COLOUR_STREAM = 15 };
enum { H264MI_TENSOR_UNSPEC_BT601 = 0, H264MI_TENSOR_UNSPEC_BT709 = 1, H264MI_TENSOR_UNSPEC_SIZE = 2 };
#define H264MI_TENSOR_COLOUR_SHIFT 8
#define H264MI_TENSOR_UNSPEC_SHIFT 12
#define H264MI_TENSOR_MODE(layout, colour, unspec) \
    ((layout) | (colour) << H264MI_TENSOR_COLOUR_SHIFT | (unspec) << H264MI_TENSOR_UNSPEC_SHIFT)
#define H264MI_TENSOR_LAYOUT(mode) ((mode) & 0xFF)
#define H264MI_TENSOR_COLOUR(mode) (((mode) >> H264MI_TENSOR_COLOUR_SHIFT) & 15)
#define H264MI_TENSOR_UNSPEC(mode) (((mode) >> H264MI_TENSOR_UNSPEC_SHIFT) & 3)
/* The colour id, 0..3, an export with `mode` uses for a picture whose SPS has
 * matrix_coefficients `matrix` (2: none given) and full-range flag `full`, over
 * a window of cw x ch pixels: the id in `mode`, or STREAM resolved as above;
 * -1 for a mode the H264SwDec tensor calls refuse.  A pure function. */
int h264mi_tensor_colour_resolve(int mode, int matrix, int full, int cw, int ch);
/* the six integers of set `id` into out; -1 for an id that is not 0..3 */
int h264mi_tensor_colour_coeffs(int id, int out[6]);
/* NextPicture, the picture exported to device memory instead of copied to the
 * host: d_dst (on the decoder's GPU, a multiple of the element size) receives
 * the tensor of `desc`, ordered on `hip_stream` as h264mi_engine_export_tensor
 * orders it (NULL: the null stream); pOutput->pOutputPicture = d_dst.  desc ==
 * NULL: RGB, fp16, scale 1/255, bias 0 over the active SPS's crop window (the
 * whole picture when croppingFlag == 0); a desc with cw == 0 takes that window
 * too.  H264SWDEC_PARAM_ERR on a bad desc or d_dst and when the backend cannot
 * export: there is no host fallback. */
H264SwDecRet H264SwDecNextPictureTensor(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                        const h264mi_tensor_desc *desc, void *d_dst, void *hip_stream);
/* The tensor resized on the GPU (resize.hip): the window of `t`,
 * as the uint8 samples above, filtered per plane to oh x ow samples (1 ..
 * 16384 each, odd allowed) by an antialiased triangle filter in integer
 * arithmetic -- bilinear with half-pixel centres when upscaling, the triangle
 * widened by the ratio when downscaling, at most 32 source samples per output
 * and axis --, then converted as above: (3 | 1, oh, ow) elements.  With (oh,
 * ow) == (ch, cw) the bytes are those of the unresized tensor.  `filter` is
 * H264MI_RESIZE_TRIANGLE or H264MI_RESIZE_BICUBIC; other values (1 and -1
 * among them: reserved) are refused.
 *
 * H264MI_RESIZE_BICUBIC is the antialiased bicubic filter of PIL's
 * BICUBIC and torch's F.interpolate(mode="bicubic", antialias=True): the Keys
 * kernel with a = -0.5, its support stretched by the ratio when downscaling, at
 * most 16 source samples per output and axis (64 taps), in integers.  One
 * axis, n source samples -> m outputs (the mapping is the triangle's):
 *   R = 2 max(m, n); output j has C = (2 j + 1) n - m; source sample k, 0 <= k
 *   < n, is at distance d = |2 m k - C| and is kept where d < 2 R (taps outside
 *   the window are dropped, not clamped; zero weights at d == R are kept);
 *   w  = 3 d^3 - 5 R d^2 + 2 R^3              (d < R)
 *      = -d^3 + 5 R d^2 - 8 R^2 d + 4 R^3     (R <= d < 2 R)     exact in 64 bits;
 *   w' = w >> s, s = max(0, bitlen(2 R^3) - 16) (arithmetic shift: floor);
 *   W  = sum w' (> 0);  q_k = floor((w'_k 16384 + W / 2) / W), which may be
 *   negative; 16384 - sum q_k is added to the first tap of largest w'.
 * Two passes, signed, with one clamp at the end:
 *   t   = (sum_k qx_k s[row][k] + 128) >> 8                 (arithmetic; an int16)
 *   out = clamp((sum_l qy_l t[l] + (1 << 19)) >> 20, 0, 255)
 * It is within 0.5 + 1/32 of that torch operator in float64, clamped to 0 ..
 * 255, and (oh, ow) == (ch, cw) still gives the unresized tensor's bytes.
 * Everywhere below, "32 source samples per output and axis" is 16 under this
 * filter.  The letterbox fit (h264mi_letterbox_fit) is the same function for
 * both filters -- its minor axis is raised to ceil(n / 32) --, so a window whose
 * fitted content would exceed 16 : 1 on an axis is refused under BICUBIC. */
enum { H264MI_RESIZE_TRIANGLE = 0, H264MI_RESIZE_BICUBIC = 2 };
typedef struct { h264mi_tensor_desc t; int ow, oh, filter; } h264mi_tensor_resize_desc;
/* NextPictureTensor with the resized tensor of `desc` (not NULL) at d_dst;
 * desc->t.cw == 0 takes the active SPS's crop window.  Otherwise as above. */
H264SwDecRet H264SwDecNextPictureTensorResized(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                               const h264mi_tensor_resize_desc *desc, void *d_dst, void *hip_stream);
/* Both calls take colour ids 0..3 and H264MI_TENSOR_COLOUR_STREAM in the
 * descriptor's mode, and refuse a bad mode (H264SWDEC_PARAM_ERR) before a
 * picture is taken from the DPB.  The colour id, 0..3, of the last tensor
 * either call delivered (GRAY: 0); -1 before the first one. */
int H264SwDecLastTensorColour(H264SwDecInst decInst);
/* Regions of interest (resize.hip): a list of boxes, each a
 * window (x, y, cw, ch) of picture `pic` of a call's picture list, every one
 * resized to the same (oh, ow) as the resized tensor above: box r is the
 * resized tensor of its window, (3 | 1, oh, ow) elements.  The descriptor's
 * own window (t.x, t.y, t.cw, t.ch) is reserved: all zero.  Each box follows
 * the resized tensor's window rules (even, inside the picture, at most 16384 a
 * side and 32 source samples per output and axis; upscaling allowed); one bad
 * box refuses the whole list.  H264MI_ROIS_MAX_PER_LAUNCH boxes go into one
 * kernel launch; a longer list takes several. */
#define H264MI_ROIS_MAX_PER_LAUNCH 32
typedef struct { int pic, x, y, cw, ch; } h264mi_roi;
/* Boxes of the picture the last H264SwDecNextPicture* call of any kind
 * delivered, valid until the next H264SwDecDecode; the DPB is not touched.
 * Every pic is 0; box coordinates are in the delivered (SPS crop) window --
 * the call adds the crop offset -- and a box lies inside it.  Box r's
 * (planes, oh, ow) elements at d_dst + r * planes * oh * ow elements, ordered
 * on `hip_stream` like H264SwDecNextPictureTensor.  Colour ids 0..3 are taken
 * as they are; H264MI_TENSOR_COLOUR_STREAM resolves from the delivered
 * picture's own VUI, by size from the crop window's size (every box gets the
 * colour the whole-picture tensor gets); H264SwDecLastTensorColour reports it.
 * H264SWDEC_PARAM_ERR for anything the export can refuse (checked before
 * anything is queued) and when the backend cannot export; H264SWDEC_OK when no
 * picture has been delivered; H264SWDEC_PIC_RDY on success. */
H264SwDecRet H264SwDecLastPictureTensorRois(H264SwDecInst decInst, const h264mi_tensor_resize_desc *desc,
                                            const h264mi_roi *rois, u32 nrois, void *d_dst, void *hip_stream);
/* Letterboxed tensors (resize.hip): the window scaled with its
 * aspect ratio kept and placed in a canvas of r.oh x r.ow (the output's shape,
 * as for the resized tensor), the rest of the canvas a constant.  The fit of a
 * cw x ch window into ow x oh is the content size and position (rw, rh, px,
 * py), in integers with 64-bit intermediates:
 *   width-bound (cw oh >= ch ow)  rw = ow, rh = (2 ch ow + cw) / (2 cw) --
 *       nearest, halves up --, raised to max(rh, ceil(ch / 32), 1), which keeps
 *       the minor axis within the resize's 32 source samples per output;
 *   height-bound (otherwise)      the same with the axes swapped;
 *   H264MI_FIT_LETTERBOX          px = (ow - rw) / 2, py = (oh - rh) / 2, floored;
 *   H264MI_FIT_LETTERBOX_TOPLEFT  px = py = 0;
 *   H264MI_FIT_STRETCH            (ow, oh, 0, 0): the resized tensor's bytes.
 * Inside the content rectangle the output is the resized tensor of the window
 * at (rh, rw), byte for byte; everywhere else the element a sample of value
 * pad[p] of plane p (R, G, B or luma; GRAY uses pad[0]) becomes under scale[p]
 * and bias[p].  pad[3] is reserved: 0.  Rules: the resized tensor's, with the
 * window judged against its content size (cw <= 32 rw, ch <= 32 rh), fit one of
 * the three, pad[3] == 0. */
enum { H264MI_FIT_STRETCH = 0, H264MI_FIT_LETTERBOX = 1, H264MI_FIT_LETTERBOX_TOPLEFT = 2 };
typedef struct { h264mi_tensor_resize_desc r; int fit; unsigned char pad[4]; } h264mi_tensor_fit_desc;
/* (rw, rh, px, py) of a cw x ch window in an ow x oh canvas into out; -1 for a
 * size below 1 or above 16384, or an unknown fit.  A pure function. */
int h264mi_letterbox_fit(int cw, int ch, int ow, int oh, int fit, int out[4]);
/* NextPictureTensorResized and LastPictureTensorRois, letterboxed: the
 * window (desc->r.t.cw == 0: the crop window), or every box, gets its own fit
 * into the canvas.  H264MI_TENSOR_COLOUR_STREAM resolves as for those calls
 * (by size: from the export window, never from the canvas), and
 * H264SwDecLastTensorColour reports it.  Return codes are theirs. */
H264SwDecRet H264SwDecNextPictureTensorFit(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                           const h264mi_tensor_fit_desc *desc, void *d_dst, void *hip_stream);
H264SwDecRet H264SwDecLastPictureTensorRoisFit(H264SwDecInst decInst, const h264mi_tensor_fit_desc *desc,
                                               const h264mi_roi *rois, u32 nrois, void *d_dst, void *hip_stream);
/* The element order of an RGB tensor: one descriptor over all
 * four pixel exports above, and a layout.  f.r.ow == 0 && f.r.oh == 0 is the
 * unresized tensor of the window f.r.t (then fit is H264MI_FIT_STRETCH, pad
 * all zero and filter 0); otherwise `f` is the fit descriptor with its own
 * rules, H264MI_FIT_STRETCH being the resized tensor.  A picture or box is the
 * same planes * rows * cols elements at the same place as in the call it
 * mirrors, with the same values:
 *   H264MI_LAYOUT_PLANAR        element (p, i, j) at index (p * rows + i) * cols + j:
 *                               that call's bytes;
 *   H264MI_LAYOUT_INTERLEAVED   element (p, i, j) at index (i * cols + j) * planes + p
 *                               (channels-last: HWC per picture, NHWC over a batch).
 * With GRAY both are the same bytes.  Other layout values are refused. */
enum { H264MI_LAYOUT_PLANAR = 0, H264MI_LAYOUT_INTERLEAVED = 1 };
typedef struct { h264mi_tensor_fit_desc f; int layout; } h264mi_tensor_layout_desc;
/* NextPictureTensor / ...Resized / ...Fit and LastPictureTensorRois / ...RoisFit
 * under a layout descriptor (not NULL): desc->f.r.t.cw == 0 takes the active
 * SPS's crop window; with boxes the window is reserved (all zero) and a size
 * is required.  H264MI_TENSOR_COLOUR_STREAM resolves as for those calls and
 * H264SwDecLastTensorColour reports it; a bad descriptor is refused before a
 * picture is taken.  Return codes are those of the calls these mirror. */
H264SwDecRet H264SwDecNextPictureTensorLayout(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                              const h264mi_tensor_layout_desc *desc, void *d_dst, void *hip_stream);
H264SwDecRet H264SwDecLastPictureTensorRoisLayout(H264SwDecInst decInst, const h264mi_tensor_layout_desc *desc,
                                                  const h264mi_roi *rois, u32 nrois, void *d_dst, void *hip_stream);
/* Where a pixel export writes: the strides of the destination,
 * in bytes, so that an export fills a clip (N, C, T, H, W), a slice of a wider
 * tensor or a tile of a canvas in place.  An item k -- a picture, a box or a
 * warp -- of planes * rows * cols elements of es bytes starts at
 *   d_out + (k / clip) * out_stride + (k % clip) * frame
 * and its element (p, i, j) lies at
 *   planar:       + p * plane + i * row + j * es
 *   interleaved:  + i * row + (j * planes + p) * es
 * NULL, or all zero with clip = 1, is the packed item of the call without a
 * descriptor, byte for byte.  Contiguous NCTHW: row = 0, frame = rows * cols *
 * es, plane = T * frame, out_stride = C * plane.
 * Rules (common/export_desc.h dest_ok; one broken rule refuses the call, nothing
 * launched): every stride, out_stride included, is a non-negative multiple of
 * es; row is at least the packed row; plane is 0 when interleaved; clip >= 1
 * divides the number of items; frame is 0 with clip = 1; reserved is 0; and no
 * two elements share an address: of the levels (row, rows), (plane, planes) if
 * planar, (frame, clip) and (out_stride, items / clip), those with a count
 * above 1, sorted by stride, each have a stride of at least the span of
 * everything below them (the packed row at the bottom, then (count - 1) *
 * stride + span).  The levels' order is free: an item stride below the plane
 * stride (clip.permute(1, 0, 2, 3)) and a frame below the row (a tile grid) are
 * legal.  The destination's total extent is the caller's business, as
 * out_stride's always was. */
typedef struct {
    int64_t row;     /* bytes between two rows; 0: packed (cols * es, interleaved: cols * planes * es) */
    int64_t plane;   /* bytes between two planes (planar only; interleaved: must be 0); 0: rows * row */
    int64_t frame;   /* bytes between two consecutive items of a clip (clip == 1: must be 0) */
    int32_t clip;    /* T >= 1: items per clip */
    int32_t reserved;/* 0 */
} h264mi_tensor_dest;
/* NextPictureTensorLayout into a strided destination (dest NULL: that call).
 * One picture is one item, so dest->clip is 1: a caller that fills a clip
 * moves d_dst itself (d_dst = clip + t * frame).  A bad descriptor is refused
 * before a picture is taken.  A backend without export_tensor_dest:
 * H264SWDEC_PARAM_ERR. */
H264SwDecRet H264SwDecNextPictureTensorDest(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                            const h264mi_tensor_layout_desc *desc, const h264mi_tensor_dest *dest,
                                            void *d_dst, void *hip_stream);
/* Affine-warped tensors (warp.hip): rotated boxes, aligned crops.
 * A warp makes (planes, oh, ow) elements from the window t.(x, y, cw, ch) of
 * one picture (even, as for every pixel export; at most 16384 a side).  Six
 * int32 coefficients m[0..5] in Q16 map an OUTPUT element to a SOURCE position
 * (the inverse map, cv2's WARP_INVERSE_MAP); sample (c, r) of the window sits
 * at (c << 16, r << 16).  For output row i, column j, in exact 64-bit integers:
 *   X = m0 j + m1 i + m2            Y = m3 j + m4 i + m5
 *   Xr = (X + 128) >> 8             Yr = (Y + 128) >> 8      (arithmetic shifts: floor)
 *   x0 = Xr >> 8, fx = Xr & 255     y0 = Yr >> 8, fy = Yr & 255
 *   v  = ((256 - fx) (256 - fy) s(x0, y0)     + fx (256 - fy) s(x0 + 1, y0)
 *       + (256 - fx) fy       s(x0, y0 + 1) + fx fy         s(x0 + 1, y0 + 1) + 32768) >> 16
 * s(c, r) is the 8-bit sample of that plane at window position (c, r): R, G or
 * B of the descriptor's colour set (4:2:0 chroma replicated, as for the tensor
 * above) or luma -- the warp filters converted samples, as the resize does.  A
 * tap outside [0, cw) x [0, ch) is judged on its own: with
 * H264MI_WARP_BORDER_CONSTANT it is the pad sample pad[p] of plane p, with
 * H264MI_WARP_BORDER_REPLICATE the sample at the clamped position; nothing
 * outside the window is ever read.  v <= 255 without a clamp, and becomes an
 * element under scale[p] and bias[p] as everywhere.  So the identity (65536, 0,
 * 0, 0, 65536, 0) at (oh, ow) == (ch, cw) gives the bytes of the unresized
 * tensor of the window, and every map with whole-sample coefficients (shifts,
 * flips, quarter turns) copies samples.  Every int32 coefficient is legal: a
 * degenerate matrix samples one point, a huge one lies outside the window
 * everywhere.  There is no antialiasing: beyond about 2 : 1 a warp aliases
 * (shrink with the resized tensor or the boxes above).
 * Rules: the element types of the tensor above; 1 <= ow, oh <= 16384; filter
 * H264MI_WARP_BILINEAR; a known border; pad[3] == 0, and pad all zero with
 * REPLICATE; layout as in h264mi_tensor_layout_desc; the window even, inside
 * the picture, at most 16384 a side; at least one warp, every pic in the
 * picture list.  One bad warp refuses the whole list. */
enum { H264MI_WARP_BILINEAR = 0 };
enum { H264MI_WARP_BORDER_CONSTANT = 0, H264MI_WARP_BORDER_REPLICATE = 1 };
typedef struct { int pic; int m[6]; } h264mi_warp;
typedef struct { h264mi_tensor_desc t; int ow, oh, filter, border; unsigned char pad[4]; int layout; } h264mi_tensor_warp_desc;
#define H264MI_WARPS_MAX_PER_LAUNCH 32
/* Warps of the picture the last H264SwDecNextPicture* call delivered, as
 * H264SwDecLastPictureTensorRois takes boxes: every pic is 0; desc->t.cw == 0
 * takes the SPS crop window, otherwise the window is relative to the crop
 * window and lies inside it -- the call adds the crop offset to the window,
 * never to the matrices, so no tap reaches a sample outside the delivered
 * picture.  Warp r's (planes, oh, ow) elements at d_dst + r * planes * oh * ow
 * elements.  H264MI_TENSOR_COLOUR_STREAM resolves from the delivered picture's
 * VUI (by size: from the crop window) and H264SwDecLastTensorColour reports
 * it.  Return codes are H264SwDecLastPictureTensorRois's. */
H264SwDecRet H264SwDecLastPictureTensorWarps(H264SwDecInst decInst, const h264mi_tensor_warp_desc *desc,
                                             const h264mi_warp *warps, u32 nwarps, void *d_dst, void *hip_stream);
/* Picture statistics (stats.hip): answers about a picture without
 * exporting it -- a scene cut, a black or frozen frame, a clip's mean and
 * standard deviation, a box's colour histogram, the PSNR of two decodes -- from
 * one pass over the frame slot, as exact integers.  An item is one window (x,
 * y, cw, ch: the pixel exports' rules -- even, inside the picture -- with no
 * size cap) of one picture, or one box of a box list (h264mi_roi above; the
 * descriptor's own window is then reserved: all zero).  Its result is P plane
 * records of L little-endian int64 words, contiguous; P = 1 for
 * H264MI_STATS_Y, 3 for H264MI_STATS_YUV and H264MI_STATS_RGB; L =
 * H264MI_STATS_WORDS, plus H264MI_STATS_BINS with the flag H264MI_STATS_HIST:
 *   0  count   samples of the plane in the item (U and V: (cw / 2) (ch / 2))
 *   1  sum     sum of s                    2  sumsq   sum of s^2
 *   3  min                                 4  max
 *   5  sad     sum of |s - r| against the reference picture; 0 without one
 *   6  ssd     sum of (s - r)^2; 0 without one
 *   7  reserved: 0
 *   8 .. 263   hist[v]: samples equal to v (H264MI_STATS_HIST only)
 * The samples s: Y and YUV take the stored samples of the window, chroma at
 * its own 4:2:0 resolution (not replicated); RGB takes exactly the uint8 values
 * of the unresized tensor above for `colour` = 0..3, so its statistics are
 * those of that tensor.  A reference is a second picture list of the same
 * length: item k -- box k of picture pic -- is compared with the same window
 * of reference picture k -- pic.  Every word of every record is written
 * whatever the destination held; there is no floating point, and the result
 * does not depend on the order of summation.
 * Rules: planes one of the three; flags 0 or H264MI_STATS_HIST; reserved 0;
 * colour 0..3 with RGB and 0 otherwise (the H264SwDec call also takes
 * H264MI_TENSOR_COLOUR_STREAM with RGB); the window, or every box, even and
 * inside the picture; one bad box refuses the list. */
enum { H264MI_STATS_Y = 0, H264MI_STATS_YUV = 1, H264MI_STATS_RGB = 2 };
#define H264MI_STATS_HIST  1        /* flags */
#define H264MI_STATS_WORDS 8
#define H264MI_STATS_BINS  256
typedef struct { int x, y, cw, ch, planes, colour, flags, reserved; } h264mi_stats_desc;
/* the int64 words of one item, P * L; 0 for a bad planes / flags.  A pure function. */
size_t h264mi_stats_item_words(const h264mi_stats_desc *desc);
/* Statistics of the picture the last H264SwDecNextPicture* call delivered, as
 * H264SwDecLastPictureTensorRois takes boxes: valid until the next
 * H264SwDecDecode, the DPB is not touched.  rois == NULL (nrois 0): the
 * descriptor's window, relative to the delivered (SPS crop) window and inside
 * it, cw == 0 taking all of it; else every pic is 0 and every box is in the
 * crop window's coordinates -- the call adds the crop offset.  Item r's words
 * at d_dst + r * h264mi_stats_item_words(desc) * 8 bytes (d_dst a multiple of
 * 8), ordered on `hip_stream`.  colour == H264MI_TENSOR_COLOUR_STREAM (RGB)
 * resolves from the delivered picture's VUI -- BT.601 where it names no
 * matrix -- and H264SwDecLastTensorColour reports it.  There is no reference
 * picture here: the decoder does not hold the previously delivered picture's
 * slot, so a decoder user detects cuts from consecutive histograms.
 * Return codes are H264SwDecLastPictureTensorRois's. */
H264SwDecRet H264SwDecLastPictureStats(H264SwDecInst decInst, const h264mi_stats_desc *desc, const h264mi_roi *rois,
                                       u32 nrois, void *d_dst, void *hip_stream);
/* Motion vectors and MB side information as a device tensor (mbinfo.hip, DESIGN
 * 3.5d; elsewhere: ffmpeg's export_mvs).  The field lives on the luma 4x4-block
 * grid of the MB-aligned picture, BW = 4 * w_mbs columns by BH = 4 * h_mbs
 * rows.  Block (X, Y) belongs to MB (X >> 2, Y >> 2), record (Y >> 2) * w_mbs +
 * (X >> 2) of the picture's MbRec batch (include/h264mi_records.h); with (x, y)
 * = (X & 3, Y & 3) it is the record's z-scan block b = (y >> 1) * 8 + (x >> 1)
 * * 4 + (y & 1) * 2 + (x & 1), in 8x8 partition b >> 2.  A channel is one
 * integer v per block, of record r:
 *   MVX, MVY    r.mv[b][0], r.mv[b][1] (quarter-pel) of MBT_INTER / MBT_SKIP; else 0
 *   REF_IDX     MBT_INTER: (r.refidx >> 4 * (b >> 2)) & 15; MBT_SKIP: 0; else -1
 *   REF_SLOT    r.ref[b >> 2] of MBT_INTER / MBT_SKIP; else -1
 *   MB_TYPE     r.type (MBT_*, 0..4)
 *   QP          r.qp
 *   INTRA_MODE  MBT_I4x4: Intra4x4PredMode of the block, (r.i4[b >> 1] >> (b & 1)
 *               * 4) & 15; MBT_I16: 16 + (r.pred & 3); else -1
 *   CODED       bit b of r.cbits
 *   SLICE       r.slice
 * A record whose type byte is 255 carries no information (a frame slot no
 * picture was decoded into, or one filled by a slot copy): MVX, MVY and CODED
 * are 0 there, every other channel -1.
 * The window (bx, by, bw, bh) is in blocks, anywhere inside BW x BH; ch[0 ..
 * nch) are channel ids, any order, repeats allowed.  Elements: H264MI_TENSOR_I16
 * (v's low 16 bits; scale and bias ignored) or F16 / BF16 / F32,
 * fma((float)v, scale[c], bias[c]) of channel position c, converted as for
 * h264mi_tensor_desc; U8 is refused. */
enum { H264MI_MBINFO_MVX = 0, H264MI_MBINFO_MVY = 1, H264MI_MBINFO_REF_IDX = 2, H264MI_MBINFO_REF_SLOT = 3,
       H264MI_MBINFO_MB_TYPE = 4, H264MI_MBINFO_QP = 5, H264MI_MBINFO_INTRA_MODE = 6, H264MI_MBINFO_CODED = 7,
       H264MI_MBINFO_SLICE = 8, H264MI_MBINFO_NCHANNELS = 9 };
#define H264MI_MBINFO_MAX_CH 16
typedef struct {
    int bx, by, bw, bh, nch, dtype;
    int ch[16];
    float scale[16], bias[16];
} h264mi_mbinfo_desc;
/* Keep every picture's record batch on the device until its frame slot is
 * decoded into again (on != 0; 0 frees them), from the next picture on; it
 * survives a change of picture size, and on a shared engine (h264mi_set_share)
 * it switches retention on for the engine.  H264SWDEC_PARAM_ERR when the
 * backend cannot keep records. */
H264SwDecRet H264SwDecKeepMbInfo(H264SwDecInst decInst, u32 on);
/* The field of the picture most recently delivered by any H264SwDecNextPicture*
 * call of the instance, as (nch, bh, bw) elements at d_dst (on the decoder's
 * GPU, a multiple of the element size), ordered on `hip_stream` as
 * h264mi_engine_export_mbinfo orders it.  The DPB is not touched: the call goes
 * with the picture, it does not replace it.  Valid until the next
 * H264SwDecDecode, like pOutputPicture.  desc->bw == 0: the blocks covering the
 * active SPS's crop window (x, y, cw, ch): bx = x >> 2, bw = ((x + cw + 3) >> 2)
 * - bx, by and bh likewise.  H264SWDEC_PIC_RDY after an export, H264SWDEC_OK
 * when no picture has been delivered (since the last H264SwDecDecode),
 * H264SWDEC_PARAM_ERR -- nothing queued -- without H264SwDecKeepMbInfo, on a
 * bad desc or d_dst and when the backend cannot export. */
H264SwDecRet H264SwDecLastPictureMbInfo(H264SwDecInst decInst, const h264mi_mbinfo_desc *desc, void *d_dst,
                                        void *hip_stream);
/* The decoded residual as a device tensor (residual.hip): the
 * prediction error the stream carries, which neither the reconstruction (clip
 * and in-loop deblocking lose it) nor a frame difference gives back.  Three
 * planes on the MB-aligned picture: Y 16 * h_mbs rows of 16 * w_mbs samples, Cb
 * and Cr 8 * h_mbs rows of 8 * w_mbs each.  A sample is one integer v, of its
 * MB's record r (include/h264mi_records.h) and its 4x4 block b, the r.cbits bit
 * index: 0..15 luma in z-scan order, 16..19 Cb, 20..23 Cr.
 *   r.type MBT_INTER, MBT_I4x4 or MBT_I16 and b in the residual mask -- the
 *   blocks with bit b of r.cbits set, all 16 luma blocks of an MBT_I16 record
 *   with bit 24 (luma DC) set, all of Cb with bit 25 and all of Cr with bit 26
 *   (chroma DC) set: v is the sample of the block's inverse transform.  The
 *   block's levels, if bit b is set, are dequantised from scan order (LevelScale
 *   of qp % 6 shifted left by qp / 6, with r.qp for luma and r.qpc for chroma;
 *   position 0 of an MBT_I16 luma block and of a chroma block carries no level);
 *   position 0 is replaced by the block's output of the I16 luma-DC transform
 *   (0 without bit 24) or of the chroma-DC transform (0 without the plane's
 *   bit); then the 4x4 inverse transform with (x + 32) >> 6, all in 32-bit
 *   integers (the reference's ProcessResidual: h264bsdProcessLumaDc,
 *   h264bsdProcessChromaDc, h264bsdProcessBlock).
 *   Every other block of those MBs, and every sample of MBT_SKIP, MBT_IPCM and
 *   type-255 ("no information") records: v = 0.  Their cbits and coef are not
 *   looked at.
 * v is clamped to [-32768, 32767]; a stream the decoder accepts stays inside
 * [-512, 511] (beyond it the picture is an error), so the clamp only makes
 * every input well defined.
 * planes: H264MI_RESID_Y one plane at full resolution; H264MI_RESID_UV two (Cb,
 * Cr) at half resolution -- x, y, cw, ch are in luma samples and must all be
 * even, the planes are ch / 2 rows of cw / 2; H264MI_RESID_YUV three at luma
 * resolution, the chroma sample of luma (X, Y) being (X >> 1, Y >> 1).  The
 * window (x, y, cw, ch) lies anywhere inside the MB-aligned picture.  Elements:
 * H264MI_TENSOR_I16 (v) or F16 / BF16 / F32, fma((float)v, scale[c], bias[c])
 * of plane position c, converted as for h264mi_tensor_desc; U8 is refused. */
enum { H264MI_RESID_Y = 0, H264MI_RESID_UV = 1, H264MI_RESID_YUV = 2 };
typedef struct { int x, y, cw, ch, planes, dtype; float scale[3], bias[3]; } h264mi_residual_desc;
/* Keep every picture's coefficient blocks, and its records, on the device until
 * its frame slot is decoded into again (on != 0; 0 frees them and leaves record
 * retention as H264SwDecKeepMbInfo set it), from the next picture on.  It costs
 * 27 blocks of 32 bytes per MB and frame slot (7.05 MB per 1080p slot); it
 * survives a change of picture size, and on a shared engine it is only ever
 * switched on.  H264SWDEC_PARAM_ERR when the backend cannot keep them. */
H264SwDecRet H264SwDecKeepResidual(H264SwDecInst decInst, u32 on);
/* The residual of the picture most recently delivered by any H264SwDecNextPicture*
 * call of the instance, as its planes at d_dst (on the decoder's GPU, a multiple
 * of the element size), ordered on `hip_stream` as h264mi_engine_export_residual
 * orders it.  The DPB is not touched.  Valid until the next H264SwDecDecode.
 * desc->cw == 0 and desc->ch == 0: the active SPS's crop window.
 * H264SWDEC_PIC_RDY after an export, H264SWDEC_OK when no picture has been
 * delivered (since the last H264SwDecDecode), H264SWDEC_PARAM_ERR -- nothing
 * queued -- without H264SwDecKeepResidual, on a bad desc or d_dst and when the
 * backend cannot export. */
H264SwDecRet H264SwDecLastPictureResidual(H264SwDecInst decInst, const h264mi_residual_desc *desc, void *d_dst,
                                          void *hip_stream);
/* Accumulated motion as a device tensor (accmv.hip): every luma
 * sample traced back, hop by hop, through the pictures it was predicted from to
 * its position in the key picture of its GOP -- what compressed-domain models
 * (CoViAR and its descendants) train on instead of the per-picture field above.
 * Everything lives on the luma sample grid of the MB-aligned picture, W = 16 *
 * w_mbs by H = 16 * h_mbs, both at most H264MI_ACCMV_MAX_DIM.
 * An origin map is one 32-bit word per sample, row-major, W words per row:
 * bits 0..14 JX, bit 15 zero, bits 16..30 JY, bit 31 ANCHORED.
 * One step makes picture t's map from its record batch r, per DPB slot of its
 * stream either an origin map or none, and a key flag.  Sample (x, y) belongs
 * to record (y >> 4) * w_mbs + (x >> 4) and to its z-scan block b of ((x >> 2)
 * & 3, (y >> 2) & 3) (h264mi_mbinfo_desc's b):
 *   key set: (JX, JY, ANCHORED) = (x, y, 1) for every sample; r is not read.
 *   r.type MBT_INTER or MBT_SKIP: d = ((mv[b][0] + 2) >> 2, (mv[b][1] + 2) >> 2),
 *     an arithmetic shift in 32 bits (integer-pel, round half up); q = (clamp(x
 *     + d.x, 0, W - 1), clamp(y + d.y, 0, H - 1)), the clamp of the reference
 *     fetch; s = r.ref[b >> 2].  If slot s has a map, the sample is that map's
 *     word at q, whole.  If it has none, or s >= nslots, it is (q.x, q.y, 0) and
 *     nothing is read for it.
 *   every other type (MBT_I4x4, MBT_I16, MBT_IPCM, 255): (x, y, 0); mv and ref
 *     are not looked at.
 * So ANCHORED = 1 means every hop back to the key picture was inter prediction
 * and (JX, JY) is where the sample sat in the key picture; ANCHORED = 0 means
 * the chain started at an intra MB, a slot without a map or an older key, and
 * the coordinates are those of that start.
 * An export is one integer v per sample of the window (x, y, cw, ch), in luma
 * samples anywhere inside W x H, and per channel id[0 .. nch), 1 <= nch <=
 * H264MI_ACCMV_MAX_CH, any order, repeats allowed:
 *   ADX  JX - x (the sign of MVX: one unclamped hop from a key picture gives
 *        (MVX + 2) >> 2)        ADY  JY - y
 *   JX, JY                      ANCHORED  0 or 1
 * Elements: H264MI_TENSOR_I16 (v) or F16 / BF16 / F32, fma((float)v, scale[c],
 * bias[c]) of channel position c, converted as for h264mi_tensor_desc; U8 is
 * refused. */
enum { H264MI_ACCMV_ADX = 0, H264MI_ACCMV_ADY = 1, H264MI_ACCMV_JX = 2, H264MI_ACCMV_JY = 3,
       H264MI_ACCMV_ANCHORED = 4, H264MI_ACCMV_NCHANNELS = 5 };
#define H264MI_ACCMV_MAX_CH 8
#define H264MI_ACCMV_MAX_DIM 32768
#define H264MI_ACCMV_MAX_SLOTS 32      /* slots a step takes maps for */
typedef struct {
    int x, y, cw, ch, nch, dtype;
    int id[8];
    float scale[8], bias[8];
} h264mi_accmv_desc;
/* Keep the origin map of every picture, per frame slot, on the device (on != 0;
 * 0 frees them), from the next picture on: 1024 bytes per MB and slot (8.36 MB
 * per 1080p slot) and one gather launch per picture.  It survives a change of
 * picture size, and on a shared engine it is only ever switched on.
 * H264SWDEC_PARAM_ERR when the backend cannot keep them. */
H264SwDecRet H264SwDecKeepAccMotion(H264SwDecInst decInst, u32 on);
/* The accumulated motion of the picture most recently delivered by any
 * H264SwDecNextPicture* call of the instance, as (nch, ch, cw) elements at d_dst
 * (on the decoder's GPU, a multiple of the element size), ordered on
 * `hip_stream` as h264mi_engine_export_accmv orders it.  The DPB is not touched.
 * Valid until the next H264SwDecDecode.  desc->cw == 0 and desc->ch == 0: the
 * active SPS's crop window.  The return codes are H264SwDecLastPictureMbInfo's
 * (H264SWDEC_PARAM_ERR also without H264SwDecKeepAccMotion). */
H264SwDecRet H264SwDecLastPictureAccMotion(H264SwDecInst decInst, const h264mi_accmv_desc *desc, void *d_dst,
                                           void *hip_stream);
/* The accumulated residual as a device tensor (accres.hip): every
 * sample of the current picture minus its origin in the key picture of its
 * GOP, cur(p) - key(J(p)) -- the third input of CoViAR-style models beside the
 * key picture's pixels and the accumulated motion above.
 * Everything lives on the MB-aligned picture, W = 16 * w_mbs by H = 16 * h_mbs.
 * A frame is a picture in the engine's slot layout (h264mi_records.h): luma
 * rows W bytes apart, then Cb, then Cr, each 8 * h_mbs rows H264MI_CPITCH(w_mbs)
 * bytes apart, H264MI_SLOT_BYTES(w_mbs, h_mbs) in all.
 * Inputs per picture: the current frame C, a key frame K or none, and an origin
 * map M in h264mi_accmv_desc's word format.  For luma sample (x, y), m = M[y *
 * W + x] gives JX, JY and A = ANCHORED; a word with JX >= W or JY >= H is
 * clamped to W - 1 / H - 1 (the engine's maps never hold one: the clamp makes
 * the stateless call well defined, and nothing outside K is ever read).
 * planes:
 *   H264MI_ACCRES_Y    one plane, v = C.Y[y][x] - K.Y[JY][JX].
 *   H264MI_ACCRES_UV   two planes (Cb, Cr) at half resolution: x, y, cw, ch
 *                      must be even; chroma sample (cx, cy) uses the word of
 *                      luma (2 cx, 2 cy), v = C.Cb[cy][cx] - K.Cb[JY >> 1][JX >> 1],
 *                      Cr the same.
 *   H264MI_ACCRES_YUV  three planes at luma resolution: Y as above, and at (x,
 *                      y) C.Cb[y >> 1][x >> 1] - K.Cb[JY >> 1][JX >> 1] with that
 *                      sample's own word, Cr the same.
 *   H264MI_ACCRES_RGB  three planes at luma resolution: v_c = rgb_c(C at (x, y))
 *                      - rgb_c(K at (JX, JY)), chroma sited as for YUV, rgb_c the
 *                      integer conversion of colour id `colour` in 0..3 (the ids
 *                      and arithmetic of h264mi_tensor_colour_coeffs);
 *                      H264MI_TENSOR_COLOUR_STREAM is refused.
 * `colour` must be 0..3 whatever the planes.  unanchored: H264MI_ACCRES_KEY
 * (0): (JX, JY) is used whatever A says -- CoViAR's convention, an intra sample
 * pretends it came from its own position; H264MI_ACCRES_ZERO (1): v = 0 where
 * A = 0.  Without a key frame every v is 0.
 * v lies in -255..255.  Elements: H264MI_TENSOR_I16 (v) or F16 / BF16 / F32,
 * fma((float)v, scale[c], bias[c]) of plane position c, converted as for
 * h264mi_tensor_desc; U8 is refused.  The window (x, y, cw, ch) lies anywhere
 * inside W x H, both at most H264MI_ACCMV_MAX_DIM. */
enum { H264MI_ACCRES_Y = 0, H264MI_ACCRES_UV = 1, H264MI_ACCRES_YUV = 2, H264MI_ACCRES_RGB = 3 };
enum { H264MI_ACCRES_KEY = 0, H264MI_ACCRES_ZERO = 1 };
#define H264MI_ACCRES_MAX_KEYS 8
typedef struct {
    int x, y, cw, ch, planes, dtype, colour, unanchored;
    float scale[3], bias[3];
} h264mi_accres_desc;
/* (The export is an engine-level call for now: h264mi_accres_device and
 * h264mi_engine_keep_accres / _export_accres below; there is no H264SwDec call.) */
/* The two fields above resized on the GPU (field_resize.hip): the
 * window's integer field filtered to oh x ow samples per channel or plane, so
 * that motion and residual arrive at a network's input size the way the pixels
 * do (h264mi_tensor_resize_desc).  `f` is the unresized export's descriptor.
 * Source samples: s[y][x] is the integer v that export defines for the channel
 * or plane on the window's own grid -- accmv: cw x ch samples, |v| <= 32767;
 * accres Y / YUV / RGB: cw x ch samples, |v| <= 255, after the `unanchored`
 * policy (a zeroed sample is a source sample 0); accres UV: the half-resolution
 * grid, cw / 2 x ch / 2.  A picture without a key is all zeros.
 * Per axis, n source samples -> m outputs, h264mi_tensor_resize_desc's taps:
 * R = 2 max(m, n); output j has C = (2 j + 1) n - m; source sample k, 0 <= k <
 * n, weighs w_k = R - |2 m k - C| where that is positive; q_k = (w_k * 16384 +
 * W / 2) / W with W = sum w_k, and 16384 - sum q_k goes to the first tap of
 * largest weight; at most 64 taps (n <= 32 m).
 * Both axes, no intermediate rounding:
 *   acc = sum_l qy_l * (sum_k qx_k * s[l][k])   (the inner sum is below 2^29 in
 *         magnitude, acc below 2^43; exact integers, any order)
 *   r   = (acc + 2^23) >> 24, an arithmetic shift: the filtered value in units
 *         of 1 / 16, |r| < 2^19.
 * Elements: H264MI_TENSOR_I16 (r + 8) >> 4, arithmetic (halves go up); F16 /
 * BF16 / F32 fma((float)r * 0.0625f, scale[c], bias[c]) ((float)r * 0.0625f is
 * exact), converted as for h264mi_tensor_desc; U8 is refused.  With (oh, ow) ==
 * the grid every output has the single tap 16384, r = 16 s, and the bytes are
 * the unresized export's.
 * Rules: f's own; filter == H264MI_RESIZE_TRIANGLE (the fields have no bicubic
 * form: H264MI_RESIZE_BICUBIC is refused here); 1 <= ow, oh <= 16384; the
 * source grid at most 16384 a side and at most 32 ow by 32 oh. */
typedef struct { h264mi_accmv_desc  f; int ow, oh, filter; } h264mi_accmv_resize_desc;
typedef struct { h264mi_accres_desc f; int ow, oh, filter; } h264mi_accres_resize_desc;
/* H264SwDecLastPictureAccMotion with the resized field of `desc` (not NULL), as
 * (nch, oh, ow) elements at d_dst; desc->f.cw == 0 and desc->f.ch == 0: the
 * active SPS's crop window.  Retention comes from H264SwDecKeepAccMotion; the
 * return codes are H264SwDecLastPictureAccMotion's. */
H264SwDecRet H264SwDecLastPictureAccMotionResized(H264SwDecInst decInst, const h264mi_accmv_resize_desc *desc,
                                                  void *d_dst, void *hip_stream);
/* Extension (no reference counterpart): where an instance's time went, in
 * seconds since H264SwDecInit -- host parse (NAL extraction, headers, CAVLC /
 * MB layer, DPB, concealment), record upload + kernel launch, waiting for the
 * device in NextPicture, and the output copy -- plus pictures output.  Any
 * pointer may be NULL. */
H264SwDecRet H264SwDecGetTiming(H264SwDecInst decInst, double *parse_s, double *submit_s, double *wait_s,
                                double *copy_s, u32 *pictures);
/* Extension: per-GPU shared engine for concurrent instances (threads) of one
 * process.  With lanes >= 2 (or H264MI_SHARE=lanes in the environment), the
 * instances decoding pictures of the same size on one device share one
 * engine of `lanes` streams (one such engine per picture size): each H264SwDecDecode hands its picture to the
 * batch being collected and returns once a launch took it; a batch launches
 * when every attached instance has submitted or 1 ms (H264MI_SHARE_WAIT_US)
 * after its first picture, as one k_prep + k_wgpp launch.  Set before the instances are
 * configured (their first picture); 0 turns it off.  Outputs, order and
 * error reporting per instance are unchanged.  The reference's model is N
 * independent instances (TestBenchMultipleInstance.c:134-305). */
int h264mi_set_share(int lanes);
/* batches / pictures launched by device's shared engine; returns the
 * instances attached (0: none) */
int h264mi_share_stats(int device, unsigned long long *batches, unsigned long long *pictures);
/* diagnostics, host CPU attribution of this process: the CPU seconds of the
 * speculative-parse worker threads that have exited (threads named
 * "h264mi-spec"), and how many were started */
int h264mi_host_thread_stats(double *spec_worker_cpu_s, unsigned long long *workers_started);

/* ---------------------------------------------------------------------- */
/* 2. Broadway glue (reference Decoder/src/Decoder.c:44-185, make.py:39)   */
/* ---------------------------------------------------------------------- */
typedef void (*broadway_headers_cb)(void *user);
typedef void (*broadway_picture_cb)(void *user, u8 *buffer, u32 width, u32 height);

void broadwaySetCallbacks(broadway_headers_cb on_headers, broadway_picture_cb on_picture, void *user);
u32  broadwayInit(void);                    /* Decoder.c:178 */
u8  *broadwayCreateStream(u32 length);      /* Decoder.c:58  */
void broadwayPlayStream(u32 length);        /* Decoder.c:67  */
void broadwayExit(void);                    /* Decoder.c:88  */
u32  broadwayGetMajorVersion(void);         /* Decoder.c:164 */
u32  broadwayGetMinorVersion(void);         /* Decoder.c:169 */

/* ---------------------------------------------------------------------- */
/* 3. Batched reconstruction engine (MI355X hot path)                      */
/* ---------------------------------------------------------------------- */
typedef struct h264mi_engine h264mi_engine;

/* Engine C-ABI revision, bumped whenever a function or a record field keeps
 * its name but changes meaning, so that an integration built against an
 * older revision can refuse to run (compare H264MI_ENGINE_ABI at build time
 * with h264mi_engine_abi() at run time):
 *   5  h264mi_engine_frame_bytes returns the packed I420 size of one picture;
 *      slots are h264mi_engine_slot_bytes apart and their chroma rows
 *      h264mi_engine_chroma_pitch (H264MI_CPITCH) apart -- before, it was the
 *      slot stride of unpadded I420 slots
 *   6  PicDesc.flags bit 3 (PD_NO_DEBLOCK) for device-resident callers */
#define H264MI_ENGINE_ABI 6
int h264mi_engine_abi(void);

/* Reconstruction engine for `nstreams` independent streams of one size
 * (w_mbs x h_mbs macroblocks), each with `nslots` frame slots in HBM. */
h264mi_engine *h264mi_engine_create(int device, int w_mbs, int h_mbs, int nstreams, int nslots);
void h264mi_engine_destroy(h264mi_engine *e);

/* Reconstruct one picture per listed stream (host-resident record batches):
 * recs[i] -> w*h MbRec (96 B each), coefs[i] -> ncoef[i] int16x16 blocks. */
int h264mi_engine_decode(h264mi_engine *e, int npics, const int *stream, const int *cur_slot,
                         const void *const *recs, const int16_t *const *coefs, const uint32_t *ncoef);

/* Shape hint for the next launch of a device-resident batch (the host path,
 * h264mi_engine_decode, derives it from the records itself): 1 if some picture
 * of the batch has more than half its MBs intra, 0 if none.  P-picture
 * launches then run 4-wave row workgroups (2 MC waves, every MB row resident
 * at once), intra-heavy ones 5-wave workgroups (3 MC waves); without a hint
 * the launch uses 3.  A hint covers one launch.  Returns 0, or -1 on a bad
 * argument. */
int h264mi_engine_hint_intra(h264mi_engine *e, int intra_heavy);
/* MC waves per row workgroup of the last launch: 2 or 3, or 6 for an
 * intra-heavy launch whose rows all fit two workgroups per CU (diagnostics) */
int h264mi_engine_last_mc_waves(h264mi_engine *e);
/* the next frame-pipelined launch's dependency mode: 1 whole MB rows of the
 * earlier steps' pictures (MbRec.i4 rows from h264mi_capture), 2 (MB row, MB
 * column) cells (geometry in the kernel), 0 the engine's default
 * (H264MI_DEP_MODE=rows|cols, default rows); last_deps: the mode the last
 * launch ran (0: one step, no dependency) */
int h264mi_engine_hint_deps(h264mi_engine *e, int mode);
int h264mi_engine_last_deps(h264mi_engine *e);

/* Neighbour-based error concealment on the device (ConcealMb's intra branch,
 * h264bsd_conceal.c:337-579, replaces the host pass over a copy of the
 * picture): the MBs order[0..n) of stream `stream`'s slot `slot` -- which holds
 * the picture's decoded MBs reconstructed with the loop filter off -- are
 * concealed in place in that order, behind the work already queued;
 * decoded[0..w*h) flags the decoded MBs.  Inputs are copied before return.
 * 0, or -1 on a bad argument / HIP error.  The H264SwDec* path uses it for I
 * pictures with lost MBs (H264MI_HOST_CONCEAL=1: the host path instead). */
int h264mi_engine_conceal(h264mi_engine *e, int stream, int slot, const int *order, int n,
                          const uint8_t *decoded);
/* diagnostics: k_conceal launches in this process */
unsigned long long h264mi_conceal_launches(void);
/* diagnostics: engines of H264SwDec* instances taken from the pool of
 * released ones (H264MI_ENGINE_POOL) / newly created, in this process */
void h264mi_engine_pool_stats(unsigned long long *reused, unsigned long long *created);
/* frees every released engine and pinned output frame the pools hold (what
 * instances still use is not touched; the library also drains at unload);
 * returns the engines freed.  The pinned-frame pool keeps at most
 * H264MI_HOST_POOL_MB (default 256) MB. */
int  h264mi_pool_drain(void);
/* pooled engines / pinned bytes held now */
void h264mi_pool_held(int *engines, size_t *pinned_bytes);

/* Device-resident variant (records already in HBM; kernel-only timing):
 * d_recs = npics*w*h MbRec in batch order with coefficient offsets relative
 * to d_coef, d_pics = npics PicDesc. */
int h264mi_engine_decode_device(h264mi_engine *e, int npics, const void *d_recs, const int16_t *d_coef,
                                const void *d_pics);
/* Same, with the NEXT batch named (device pointers as above; it must be the
 * batch of the following decode_device* call): this launch's tail
 * workgroups compute the next batch's deblocking records and residuals as its
 * own MB rows drain, so that batch needs no k_prep launch of its own. */
int h264mi_engine_decode_device_next(h264mi_engine *e, int npics, const void *d_recs, const int16_t *d_coef,
                                     const void *d_pics, const void *next_recs, const int16_t *next_coef,
                                     const void *next_pics);
/* Frame-pipelined batch: P consecutive pictures of each of S streams in one
 * launch, descriptors step-major (j * S + s), every PicDesc.rec_base relative
 * to d_recs.  A picture reading a slot that an earlier picture of the batch
 * reconstructs waits, per 128-B line of its reference windows, for those rows
 * to be final (device row tags), so the later picture's top rows overlap the
 * earlier one's bottom rows.  The caller guarantees that no picture of the
 * batch writes a slot an earlier picture of the batch reads or writes.
 * P <= the engine's steps (h264mi_engine_set_steps, 1..H264MI_MAX_STEPS;
 * default 1; more than 1 needs at most 32 frame slots per stream). */
int h264mi_engine_decode_device_steps(h264mi_engine *e, int S, int P, const void *d_recs, const int16_t *d_coef,
                                      const void *d_pics, const void *next_recs, const int16_t *next_coef,
                                      const void *next_pics);
/* The same, naming the next batch's step count next_P (1 .. steps) when it
 * differs from P: the next batch's k_prep runs in this launch's tail over its
 * S * next_P pictures (a plan mixing one- and two-step launches). */
int h264mi_engine_decode_device_steps_next(h264mi_engine *e, int S, int P, const void *d_recs,
                                           const int16_t *d_coef, const void *d_pics, const void *next_recs,
                                           const int16_t *next_coef, const void *next_pics, int next_P);
#define H264MI_MAX_STEPS 4
int h264mi_engine_set_steps(h264mi_engine *e, int steps);

int  h264mi_engine_read(h264mi_engine *e, int stream, int slot, uint8_t *dst);   /* D2H I420 */
/* D2H of a slot as RGBA (w*16 * h*16 * 4 bytes), converted on the GPU
 * (DecoderPost.js yuv2rgbcalc :514-560 per pixel) */
int  h264mi_engine_read_rgba(h264mi_engine *e, int stream, int slot, uint8_t *dst);
/* the conversion kernel on device buffers: npics MB-aligned I420 pictures
 * of width x height (multiples of 16) at d_i420 + k * in_stride ->
 * d_rgba + k * out_stride; asynchronous on `hip_stream` (NULL: null stream) */
int  h264mi_yuv2rgba_device(const void *d_i420, void *d_rgba, int width, int height, int npics,
                            size_t in_stride, size_t out_stride, void *hip_stream);
/* the same with the chroma rows cpitch bytes apart (an engine slot:
 * h264mi_engine_chroma_pitch; the packed form above is cpitch = width / 2) */
int  h264mi_yuv2rgba_device_pitch(const void *d_i420, void *d_rgba, int width, int height, int cpitch, int npics,
                                  size_t in_stride, size_t out_stride, void *hip_stream);
/* display cropping on the device (crop.hip): the window (x, y, cw, ch -- luma
 * pixels, all even, x + cw <= width, y + ch <= height) of npics pictures of
 * width x height pixels (even) at d_in + k * in_stride, chroma rows cpitch
 * bytes apart (an engine slot, or packed I420 with cpitch = width / 2), packed
 * at d_out + k * out_stride: rgba == 0 I420 in the layout of the reference
 * testbench's CropPicture (cw * ch * 3 / 2 bytes, DecTestBench.c:588-666),
 * else RGBA (cw * ch * 4 bytes, the crop of h264mi_yuv2rgba_device's output;
 * d_out and, for npics > 1, out_stride multiples of 8).  Device pointers,
 * asynchronous on `hip_stream`.  -1 on a bad argument, nothing launched. */
int  h264mi_crop_device_pitch(const void *d_in, void *d_out, int width, int height, int cpitch, int x, int y,
                              int cw, int ch, int rgba, int npics, size_t in_stride, size_t out_stride,
                              void *hip_stream);
/* D2H of the crop window of a slot, I420 or RGBA as above: waits for the
 * engine's launches, crops into a staging buffer, one contiguous copy */
int  h264mi_engine_read_crop(h264mi_engine *e, int stream, int slot, int x, int y, int cw, int ch, int rgba,
                             uint8_t *dst);
/* pictures as planar tensors on the device (tensor.hip, h264mi_tensor_desc
 * above): the npics pictures of width x height pixels (even) that start
 * in_offsets[k] bytes (a host array; any order, repeats allowed) after d_in,
 * chroma rows cpitch bytes apart as for h264mi_crop_device_pitch, whose window
 * rules apply; picture k's (planes, ch, cw) elements at d_out + k * out_stride.
 * d_out and out_stride are multiples of the element size; where they and the
 * row bytes are multiples of 16 a lane stores 16 bytes at a time.  Nothing
 * outside the planes * ch * cw elements of each picture is written.  Device
 * pointers, asynchronous on `hip_stream`.  -1 on a bad argument, nothing
 * launched.  This call and the three engine-level calls below take the colour
 * ids 0..3 in desc->mode and refuse H264MI_TENSOR_COLOUR_STREAM: they know no
 * stream. */
int  h264mi_tensor_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                int cpitch, const h264mi_tensor_desc *desc, void *d_out, size_t out_stride,
                                void *hip_stream);
/* the slots (streams[k], slots[k]), k < n, of an engine as tensors in the
 * caller's memory on the engine's GPU, without any host synchronisation: the
 * export sees every launch queued on the engine before the call, starts only
 * after the work already queued on `hip_stream` (NULL: the null stream), and
 * work queued on `hip_stream` after the call sees the finished tensors; a
 * later launch that overwrites one of the slots waits for the export.  -1 on
 * a bad stream, slot or desc, or when d_out is not on the engine's device. */
int  h264mi_engine_export_tensor(h264mi_engine *e, int n, const int *streams, const int *slots,
                                 const h264mi_tensor_desc *desc, void *d_out, size_t out_stride, void *hip_stream);
/* the two calls above with the resized tensor of an h264mi_tensor_resize_desc:
 * picture k's (planes, oh, ow) elements at d_out + k * out_stride, nothing
 * else written.  Stateless (the filter taps are derived in the kernel): no
 * device allocation, no copy, no host synchronisation.  -1, nothing launched,
 * also for ow or oh outside 1 .. 16384, a window more than 32 times
 * (H264MI_RESIZE_BICUBIC: 16 times) the output on an axis, or a filter that is
 * neither H264MI_RESIZE_TRIANGLE nor H264MI_RESIZE_BICUBIC. */
int  h264mi_tensor_resize_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                       int cpitch, const h264mi_tensor_resize_desc *desc, void *d_out,
                                       size_t out_stride, void *hip_stream);
int  h264mi_engine_export_tensor_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                         const h264mi_tensor_resize_desc *desc, void *d_out, size_t out_stride,
                                         void *hip_stream);
/* the resized export over a list of regions of interest (h264mi_roi above):
 * box r, the window rois[r].(x, y, cw, ch) of picture rois[r].pic of the
 * picture list (in_offsets, or streams / slots), resized to desc->(oh, ow):
 * its (planes, oh, ow) elements at d_out + r * out_stride, nothing else
 * written.  The bytes of box r are those h264mi_tensor_resize_device_pitch
 * gives for the same window and size.  desc->t's window is reserved (all zero);
 * `rois` is a host array, read before the call returns.  One kernel launch per
 * H264MI_ROIS_MAX_PER_LAUNCH boxes, and for the engine call one ordering of the
 * two streams however many boxes there are.  -1, nothing launched, when any
 * box or anything else is bad, d_out in no device's memory included. */
int  h264mi_tensor_rois_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                     int cpitch, const h264mi_tensor_resize_desc *desc, const h264mi_roi *rois,
                                     int nrois, void *d_out, size_t out_stride, void *hip_stream);
int  h264mi_engine_export_tensor_rois(h264mi_engine *e, int n, const int *streams, const int *slots,
                                      const h264mi_tensor_resize_desc *desc, const h264mi_roi *rois, int nrois,
                                      void *d_out, size_t out_stride, void *hip_stream);
/* the letterboxed exports (h264mi_tensor_fit_desc above): picture k's window
 * desc->r.t, or box r of the list (desc->r.t's window reserved, all zero),
 * fitted into the canvas desc->r.(oh, ow): (planes, oh, ow) elements at d_out +
 * k (or r) * out_stride, every one of them written -- the content rectangle
 * with the bytes h264mi_tensor_resize_device_pitch gives for that window at
 * the content size, the rest with the pad element -- and nothing else.  One
 * kernel launch per H264MI_ROIS_MAX_PER_LAUNCH pictures or boxes; for the
 * engine calls one ordering of the two streams per call.  -1, nothing
 * launched, when any box or anything else is bad, d_out in no device's memory
 * included. */
int  h264mi_tensor_fit_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                    int cpitch, const h264mi_tensor_fit_desc *desc, void *d_out, size_t out_stride,
                                    void *hip_stream);
int  h264mi_tensor_rois_fit_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                         int cpitch, const h264mi_tensor_fit_desc *desc, const h264mi_roi *rois,
                                         int nrois, void *d_out, size_t out_stride, void *hip_stream);
int  h264mi_engine_export_tensor_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                                     const h264mi_tensor_fit_desc *desc, void *d_out, size_t out_stride,
                                     void *hip_stream);
int  h264mi_engine_export_tensor_rois_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                                          const h264mi_tensor_fit_desc *desc, const h264mi_roi *rois, int nrois,
                                          void *d_out, size_t out_stride, void *hip_stream);
/* the eight calls above under a layout descriptor (h264mi_tensor_layout_desc
 * above): rois == NULL and nrois == 0 is desc's window of every picture, else
 * the boxes (the window reserved, a size required).  Picture or box k occupies
 * the planes * rows * cols elements at d_out + k * out_stride the mirrored call
 * writes, and nothing else is written.  H264MI_LAYOUT_PLANAR runs that call;
 * H264MI_LAYOUT_INTERLEAVED stores the same values channels-last (GRAY: the
 * same bytes, the same kernels).  d_out and out_stride are multiples of the
 * element size; where they and a row's cols * planes * element size bytes are
 * multiples of 16, the unresized export stores 16 bytes at a time.  -1,
 * nothing launched, on a bad argument. */
int  h264mi_tensor_layout_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                       int cpitch, const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois,
                                       int nrois, void *d_out, size_t out_stride, void *hip_stream);
int  h264mi_engine_export_tensor_layout(h264mi_engine *e, int n, const int *streams, const int *slots,
                                        const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois, int nrois,
                                        void *d_out, size_t out_stride, void *hip_stream);
/* the affine-warped export (h264mi_tensor_warp_desc above) over a list of
 * warps: warp r, the matrix warps[r].m over the window desc->t of picture
 * warps[r].pic of the picture list (in_offsets, or streams / slots): its
 * (planes, oh, ow) elements, in desc->layout's order, at d_out + r *
 * out_stride, nothing else written, and nothing outside the window read.
 * `warps` is a host array, read before the call returns.  One kernel launch
 * per H264MI_WARPS_MAX_PER_LAUNCH warps, and for the engine call one ordering
 * of the two streams however many there are.  -1, nothing launched, when
 * anything is bad, d_out in no device's memory included. */
int  h264mi_tensor_warps_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                      int cpitch, const h264mi_tensor_warp_desc *desc, const h264mi_warp *warps,
                                      int nwarps, void *d_out, size_t out_stride, void *hip_stream);
int  h264mi_engine_export_tensor_warps(h264mi_engine *e, int n, const int *streams, const int *slots,
                                       const h264mi_tensor_warp_desc *desc, const h264mi_warp *warps, int nwarps,
                                       void *d_out, size_t out_stride, void *hip_stream);
/* the layout and warp calls above into a strided destination
 * (h264mi_tensor_dest above): every form they cover, the same
 * values, item k's element (p, i, j) where the descriptor puts it, and not a
 * byte written that the descriptor does not address.  dest == NULL is the call
 * above.  Everything is checked before anything is launched (dest_ok with the
 * call's items: pictures, boxes or warps); a launch's 32 items may begin and
 * end inside a clip.  Where d_out, out_stride, frame, plane, row and the packed
 * row are all multiples of 16, the unresized export stores 16 bytes at a time. */
int  h264mi_tensor_dest_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                     int cpitch, const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois,
                                     int nrois, const h264mi_tensor_dest *dest, void *d_out, size_t out_stride,
                                     void *hip_stream);
int  h264mi_tensor_warps_dest_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                           int cpitch, const h264mi_tensor_warp_desc *desc, const h264mi_warp *warps,
                                           int nwarps, const h264mi_tensor_dest *dest, void *d_out, size_t out_stride,
                                           void *hip_stream);
int  h264mi_engine_export_tensor_dest(h264mi_engine *e, int n, const int *streams, const int *slots,
                                      const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois, int nrois,
                                      const h264mi_tensor_dest *dest, void *d_out, size_t out_stride, void *hip_stream);
int  h264mi_engine_export_tensor_warps_dest(h264mi_engine *e, int n, const int *streams, const int *slots,
                                            const h264mi_tensor_warp_desc *desc, const h264mi_warp *warps, int nwarps,
                                            const h264mi_tensor_dest *dest, void *d_out, size_t out_stride,
                                            void *hip_stream);
/* picture statistics (h264mi_stats_desc above): item k -- desc's window of
 * picture k of the picture list, or with rois (a host array, read before the
 * call returns; NULL with nrois 0: none) box k of picture rois[k].pic -- as
 * h264mi_stats_item_words(desc) int64 words at d_out + k * out_stride.  d_ref /
 * ref_offsets (ref_streams / ref_slots), both NULL for none, name as many
 * reference pictures of the same size and pitch: picture k's reference is
 * reference k.  d_out and out_stride are multiples of 8, and with more than
 * one item out_stride is at least the item's bytes; nothing outside the items'
 * words is written, and every word of them is.  One small launch that fills
 * the records, then the kernel, per H264MI_ROIS_MAX_PER_LAUNCH items; any
 * number of items.  The engine call is ordered like every engine export (no
 * host synchronisation; a later decode into a named slot, reference slots
 * included, waits) and refuses H264MI_TENSOR_COLOUR_STREAM.  -1 on a bad
 * argument, nothing launched. */
int  h264mi_stats_device_pitch(const void *d_in, const size_t *in_offsets, const void *d_ref, const size_t *ref_offsets,
                               int npics, int width, int height, int cpitch, const h264mi_stats_desc *desc,
                               const h264mi_roi *rois, int nrois, void *d_out, size_t out_stride, void *hip_stream);
int  h264mi_engine_export_stats(h264mi_engine *e, int n, const int *streams, const int *slots, const int *ref_streams,
                                const int *ref_slots, const h264mi_stats_desc *desc, const h264mi_roi *rois, int nrois,
                                void *d_out, size_t out_stride, void *hip_stream);
/* the MB side-information field (h264mi_mbinfo_desc above) of npics record
 * batches of w_mbs * h_mbs MbRec each, batch k starting rec_offsets[k] bytes (a
 * host array of multiples of 96; any order, repeats allowed) after d_recs
 * (16-byte aligned): picture k's (nch, bh, bw) elements, contiguous, at d_out +
 * k * out_stride.  d_out and out_stride are multiples of the element size;
 * where they and the row bytes are multiples of 16 a lane stores 16 bytes at a
 * time.  Nothing outside the nch * bh * bw elements of each picture is written.
 * Stateless; device pointers, asynchronous on `hip_stream`.  -1 on a bad
 * argument, nothing launched.  For callers that hold their records on the
 * device (h264mi_engine_decode_device*). */
int  h264mi_mbinfo_device(const void *d_recs, const size_t *rec_offsets, int npics, int w_mbs, int h_mbs,
                          const h264mi_mbinfo_desc *desc, void *d_out, size_t out_stride, void *hip_stream);
/* record retention: on != 0 allocates one record batch per (stream, slot),
 * filled with 0xFF bytes ("no information"); from then on h264mi_engine_decode
 * and the H264SwDec* path copy each picture's records into the batch of the
 * slot it is reconstructed into (one device-to-device copy on the engine's
 * stream), so a slot's batch is that of the last reconstruction into it.  The
 * decode_device* launches retain nothing: their callers own the records.  0
 * (the default) waits for the engine's stream and frees the batches -- unless
 * h264mi_engine_keep_coefs is on, which holds them until it goes off.  Returns
 * 0, or -1 on a bad argument / HIP error. */
int  h264mi_engine_keep_records(h264mi_engine *e, int on);
/* refills the slot's batch with 0xFF bytes, behind the work queued on the
 * engine (its picture did not come from a reconstruction), and with
 * h264mi_engine_keep_accmv on resets its origin map; -1 when both retentions
 * are off or on a bad stream or slot */
int  h264mi_engine_forget_records(h264mi_engine *e, int stream, int slot);
/* the kept batches of the slots (streams[k], slots[k]), k < n, as fields in the
 * caller's memory, ordered as h264mi_engine_export_tensor orders its export (no
 * host synchronisation; a later decode into one of the slots waits for the
 * export).  -1 when retention is off, on a bad stream, slot or desc, or when
 * d_out is not on the engine's device. */
int  h264mi_engine_export_mbinfo(h264mi_engine *e, int n, const int *streams, const int *slots,
                                 const h264mi_mbinfo_desc *desc, void *d_out, size_t out_stride, void *hip_stream);
/* the residual (h264mi_residual_desc above) of npics pictures of w_mbs * h_mbs
 * MBs: picture k's record batch starts rec_offsets[k] bytes (a host array of
 * multiples of 96) after d_recs, and its records' coef indices count from
 * block coef_bases[k] (a host array) of the pool d_coef of coef_blocks blocks
 * of 16 int16 (both pointers 16-byte aligned; any order, repeats allowed).
 * Picture k's planes, contiguous, go to d_out + k * out_stride.  An MB whose
 * blocks (coef_bases[k] + r.coef + the number of bits 0..26 set in r.cbits)
 * would end beyond coef_blocks is not read and exports zeros.  d_out and
 * out_stride are multiples of the element size; where they and a plane row's
 * bytes are multiples of 16 a lane stores 16 bytes at a time.  Nothing outside
 * each picture's planes is written.  Stateless; device pointers, asynchronous
 * on `hip_stream`.  -1 on a bad argument, nothing launched. */
int  h264mi_residual_device(const void *d_recs, const size_t *rec_offsets, const void *d_coef,
                            const uint32_t *coef_bases, size_t coef_blocks, int npics, int w_mbs, int h_mbs,
                            const h264mi_residual_desc *desc, void *d_out, size_t out_stride, void *hip_stream);
/* coefficient retention: on != 0 allocates, per (stream, slot), one batch of the
 * worst case of 27 blocks of 32 bytes per MB (16 luma, 8 chroma AC, 1 luma DC,
 * 2 chroma DC; I_PCM's 12 fit) -- 7.05 MB per 1080p slot, just under 1 GB for
 * eight streams of 17 slots -- and holds the records as h264mi_engine_keep_records
 * does while it is on; from then on h264mi_engine_decode and the H264SwDec* path
 * copy each picture's blocks into the batch of the slot it is reconstructed into
 * (one more device-to-device copy on the engine's stream).  A picture with more
 * blocks than a batch holds is not kept; its slot then exports zeros, like a slot
 * nothing was decoded into and one h264mi_engine_forget_records was called for.
 * The decode_device* launches retain nothing.  0 (the default: nothing is
 * allocated or queued) waits for the engine's stream, frees the batches and
 * leaves the records to h264mi_engine_keep_records' own switch.  Returns 0, or
 * -1 on a bad argument / HIP error. */
int  h264mi_engine_keep_coefs(h264mi_engine *e, int on);
/* the kept pictures of the slots (streams[k], slots[k]), k < n, as residual
 * tensors in the caller's memory, ordered as h264mi_engine_export_mbinfo orders
 * its export (no host synchronisation; a later decode into one of the slots
 * waits for the export).  -1 when coefficient retention is off, on a bad stream,
 * slot or desc, or when d_out is not on the engine's device. */
int  h264mi_engine_export_residual(h264mi_engine *e, int n, const int *streams, const int *slots,
                                   const h264mi_residual_desc *desc, void *d_out, size_t out_stride,
                                   void *hip_stream);
/* one step of the accumulated motion (h264mi_accmv_desc above): the origin map
 * of the picture whose w_mbs * h_mbs MbRec start at d_recs (16-byte aligned),
 * W * H words at d_map_out, from the maps d_ref_maps[s], s < nslots <=
 * H264MI_ACCMV_MAX_SLOTS (a host array of device pointers; NULL: slot s has
 * none; d_ref_maps itself may be NULL when nslots is 0), or with key != 0 the
 * identity.  No map may be d_map_out.  Nothing outside d_map_out's W * H words
 * is written and nothing outside the maps' is read.  Stateless; asynchronous on
 * `hip_stream`.  -1 on a bad argument or a picture beyond H264MI_ACCMV_MAX_DIM,
 * nothing launched.  For callers that hold their records on the device. */
int  h264mi_accmv_step_device(const void *d_recs, int w_mbs, int h_mbs, const void *const *d_ref_maps, int nslots,
                              int key, void *d_map_out, void *hip_stream);
/* the channels of desc over npics origin maps, map k starting map_offsets[k]
 * bytes (a host array of multiples of 4; any order, repeats allowed) after
 * d_maps: picture k's (nch, ch, cw) elements, contiguous, at d_out + k *
 * out_stride, under the alignment rules of h264mi_mbinfo_device; nothing else
 * is written.  Stateless; asynchronous on `hip_stream`.  -1 on a bad argument,
 * nothing launched. */
int  h264mi_accmv_device(const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                         const h264mi_accmv_desc *desc, void *d_out, size_t out_stride, void *hip_stream);
/* origin-map retention: on != 0 allocates one map per (stream, slot), 1024
 * bytes per MB (8.36 MB per 1080p slot: 1.14 GB for eight streams of 17 slots),
 * each (x, y, 0); from then on h264mi_engine_decode and the H264SwDec* path
 * queue one step per picture behind its reconstruction, on the engine's stream,
 * reading the uploaded records in place.  A picture without a single MBT_INTER
 * / MBT_SKIP record is a key picture: it starts its stream's next GOP and steps
 * with the key flag.  Any other picture steps from the maps of its stream's
 * slots that were written since that key picture (the slot it is decoded into
 * excepted); a map from before it counts as none, though it stays exportable.
 * A slot's map is that of the last reconstruction into it;
 * h264mi_engine_forget_records resets it to (x, y, 0).  The decode_device*
 * launches retain nothing.  0 (the default: nothing is allocated or queued)
 * waits for the engine's stream and frees the maps.  -1 on a bad argument, a
 * picture beyond H264MI_ACCMV_MAX_DIM, more than H264MI_ACCMV_MAX_SLOTS slots or
 * a HIP error. */
int  h264mi_engine_keep_accmv(h264mi_engine *e, int on);
/* the kept maps of the slots (streams[k], slots[k]), k < n, as tensors in the
 * caller's memory, ordered as h264mi_engine_export_mbinfo orders its export (no
 * host synchronisation; a later decode into one of the slots waits for the
 * export).  -1 when retention is off, on a bad stream, slot or desc, or when
 * d_out is not on the engine's device. */
int  h264mi_engine_export_accmv(h264mi_engine *e, int n, const int *streams, const int *slots,
                                const h264mi_accmv_desc *desc, void *d_out, size_t out_stride, void *hip_stream);
/* the accumulated residual (h264mi_accres_desc above) of npics pictures of
 * w_mbs x h_mbs MBs: picture k's current frame starts cur_offsets[k] bytes
 * after d_cur, its key frame key_offsets[k] bytes after d_key -- (size_t)-1:
 * picture k has no key and is all zeros; d_key may be NULL when every picture
 * has none -- and its origin map map_offsets[k] bytes after d_maps (host arrays;
 * any order, repeats allowed; every pointer and offset a multiple of 4).
 * Picture k's (planes, ch, cw) elements go, contiguous, to d_out + k *
 * out_stride under the alignment rules of h264mi_mbinfo_device; nothing else is
 * written, and no byte outside the three planes of a frame or the W * H words
 * of a map is read.  Stateless; asynchronous on `hip_stream`.  -1 on a bad
 * argument or a picture beyond H264MI_ACCMV_MAX_DIM, nothing launched.  For
 * decode_device* callers that own frames and maps. */
int  h264mi_accres_device(const void *d_cur, const size_t *cur_offsets, const void *d_key, const size_t *key_offsets,
                          const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                          const h264mi_accres_desc *desc, void *d_out, size_t out_stride, void *hip_stream);
/* key-picture retention: nkeys in 1..H264MI_ACCRES_MAX_KEYS allocates nstreams *
 * nkeys frames (3.20 MB per 1080p key: 51 MB for eight streams with two keys
 * each); it needs h264mi_engine_keep_accmv on (-1 while that is off, and
 * switching that off switches this off).  From then on, whenever a decode
 * bumps a stream's key serial to s (h264mi_engine_keep_accmv's key-picture
 * rule), one device-to-device copy of the reconstructed slot into the stream's
 * entry s % nkeys is queued behind the reconstruction, on the engine's stream,
 * and the entry is tagged s.  The copy is queued again when something rewrites
 * the key picture in its slot: h264mi_engine_conceal on that slot, and a
 * decode into it whose inter records reference the slot itself (the second
 * pass of the H264SwDec path's concealment).  A slot whose map carries serial t exports against
 * entry t % nkeys iff t != 0 and the entry is tagged t (its key is *held*); so
 * with nkeys = 2 every picture of the previous GOP stays exportable after the
 * next key picture was decoded.  Older pictures, pictures decoded before
 * retention went on, slots nothing was decoded into, slots
 * h264mi_engine_forget_records was called for, and the pictures of a GOP whose
 * key picture's slot was decoded into again later in the key picture's own
 * batch (nothing is left to copy behind that launch) have no key and export
 * zeros.
 * The decode_device* launches retain nothing.  0 (the default: nothing is
 * allocated or queued) waits for the engine's stream and frees the frames; a
 * different nkeys starts again from nothing.  -1 on a bad argument or a HIP
 * error. */
int  h264mi_engine_keep_accres(h264mi_engine *e, int nkeys);
/* 1: the key picture of the slot's picture is held, 0: it is not (the slot
 * exports zeros), -1: retention is off or a bad stream or slot */
int  h264mi_engine_accres_held(h264mi_engine *e, int stream, int slot);
/* the accumulated residual of the slots (streams[k], slots[k]), k < n, against
 * the keys held for them, as tensors in the caller's memory, ordered as
 * h264mi_engine_export_accmv orders its export.  -1 when retention is off, on a
 * bad stream, slot or desc, or when d_out is not on the engine's device. */
int  h264mi_engine_export_accres(h264mi_engine *e, int n, const int *streams, const int *slots,
                                 const h264mi_accres_desc *desc, void *d_out, size_t out_stride, void *hip_stream);
/* h264mi_accmv_device and h264mi_accres_device with the resized fields of an
 * h264mi_accmv_resize_desc / h264mi_accres_resize_desc: the same arguments,
 * picture k's (nch | planes, oh, ow) elements, contiguous, at d_out + k *
 * out_stride.  d_out and out_stride are multiples of the element size (the
 * resized rows are short: there is no 16-byte rule); nothing else is written,
 * and nothing outside the maps' words and the frames' planes is read (every
 * pointer and offset a multiple of 4, as for the unresized calls).  -1 on a bad
 * argument, nothing launched. */
int  h264mi_accmv_resize_device(const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                                const h264mi_accmv_resize_desc *desc, void *d_out, size_t out_stride,
                                void *hip_stream);
int  h264mi_accres_resize_device(const void *d_cur, const size_t *cur_offsets, const void *d_key,
                                 const size_t *key_offsets, const void *d_maps, const size_t *map_offsets, int npics,
                                 int w_mbs, int h_mbs, const h264mi_accres_resize_desc *desc, void *d_out,
                                 size_t out_stride, void *hip_stream);
/* h264mi_engine_export_accmv and h264mi_engine_export_accres with the resized
 * fields: the same retention, ordering, held-key rule and return codes */
int  h264mi_engine_export_accmv_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                        const h264mi_accmv_resize_desc *desc, void *d_out, size_t out_stride,
                                        void *hip_stream);
int  h264mi_engine_export_accres_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                         const h264mi_accres_resize_desc *desc, void *d_out, size_t out_stride,
                                         void *hip_stream);
int  h264mi_engine_sync(h264mi_engine *e);
/* number of (launch, picture) slots flagged since the last call: residual
 * range errors (reference transform.c:181) or a bounded wait that expired;
 * flags accumulate over every launch and are collected by h264mi_engine_sync */
uint32_t h264mi_engine_errors(h264mi_engine *e);
/* the OR of the device flag words of every picture synced since the last
 * call (1 residual range, 2 / 16 / 32 bounded waits expired; with
 * H264MI_CHECK=1 the dependency checker's 64 ring data, 128 ring overwrite,
 * 256 partner region, 512 intra progress, 1024 reference rows not final) */
uint32_t h264mi_engine_error_bits(h264mi_engine *e);
/* MB rows per k_wgpp workgroup the engine launches for a batch of npics
 * pictures (1..3: by batch size, H264MI_RPW, the LDS budget) */
int  h264mi_engine_rows_per_workgroup(h264mi_engine *e, int npics);
/* duration (us) of the last batch's k_wgpp launch: us2[1] (us2[0] = 0);
 * needs H264MI_TIMING in the environment */
int  h264mi_engine_last_timing(h264mi_engine *e, float *us2);
/* per-batch kernel timing with HIP events carried by k_wgpp's dispatch
 * packet: record up to max_batches launches (0 disables); the report syncs
 * and returns the summed k_wgpp durations in *wave_us (*inter_us = 0), in
 * microseconds */
int  h264mi_engine_set_timing(h264mi_engine *e, int max_batches);
/* time only every stride-th launch (default 1) */
int  h264mi_engine_set_timing_stride(h264mi_engine *e, int stride);
int  h264mi_engine_timing_report(h264mi_engine *e, double *inter_us, double *wave_us, int *nbatches);
/* the recorded launches' k_wgpp durations one by one (us[i], in recording
 * order, at most cap); returns how many (call before timing_report, which
 * resets the record) */
int  h264mi_engine_timing_list(h264mi_engine *e, double *us, int cap);
/* diagnostics: per k_wgpp workgroup (row r of batch picture p at index
 * r * npics + p) 16 u64: wall-clock start/end (100 MHz) and shader-clock sums
 * of its phases, then 4 u64 per MB (chain stamps); enable != 0 allocates and
 * switches to the profiling kernel, out != NULL copies the last launch */
int  h264mi_engine_profile(h264mi_engine *e, int enable, unsigned long long *out, size_t n);
/* device pointer of a frame slot: I420 with the chroma rows padded to
 * h264mi_engine_chroma_pitch bytes (H264MI_CPITCH, include/h264mi_records.h),
 * slots h264mi_engine_slot_bytes apart */
void *h264mi_engine_frame_ptr(h264mi_engine *e, int stream, int slot);
/* diagnostics: name of the last batch's reconstruction kernel ("k_wgpp";
 * "" before the first batch) */
const char *h264mi_engine_kernel(h264mi_engine *e);
/* packed I420 bytes of one picture (h264mi_engine_read's output) */
size_t h264mi_engine_frame_bytes(h264mi_engine *e);
size_t h264mi_engine_slot_bytes(h264mi_engine *e);
int    h264mi_engine_chroma_pitch(h264mi_engine *e);

/* MB-record capture: run the host parser over a whole Annex-B stream and keep
 * every picture's record batch (the §8d "pre-parsed MB-record batches"). */
typedef struct h264mi_capture h264mi_capture;
h264mi_capture *h264mi_capture_stream(const uint8_t *buf, size_t len, int no_reorder);
int  h264mi_capture_info(const h264mi_capture *c, int *w_mbs, int *h_mbs, int *nslots, int *npics, int *errors);
int  h264mi_capture_picture(const h264mi_capture *c, int i, const void **rec, const int16_t **coef,
                            uint32_t *ncoef, int *cur_slot, uint64_t *alg_ref_bytes);
int  h264mi_capture_stats(const h264mi_capture *c, int i, uint32_t *n_inter, uint32_t *n_intra, uint32_t *n_coded);
/* picture i's reference footprint in whole 128-B lines (distinct lines of
 * each reference slot the k_wgpp MC windows touch, x 128): the line-granular
 * reference traffic beside alg_ref_bytes' bytes used (measurement helper; no
 * reference counterpart) */
int  h264mi_capture_ref_lines(const h264mi_capture *c, int i, uint64_t *ref_line_bytes);
void h264mi_capture_free(h264mi_capture *c);

/* Device memory helpers for the device-resident path (HIP device pointers).
 * h264mi_device_alloc allocates on the calling thread's CURRENT HIP device;
 * a multi-GPU caller uses the engine-scoped forms below instead. */
void *h264mi_device_alloc(size_t bytes);
int   h264mi_device_free(void *p);
int   h264mi_copy_h2d(void *dst, const void *src, size_t bytes);
/* Engine-scoped: memory on the engine's own GPU whatever the caller's current
 * device (one process per GPU, TestBenchMultipleInstance.c:134-305 style
 * independent instances); copy_h2d refuses a destination on another GPU. */
int   h264mi_engine_device(const h264mi_engine *e);
void *h264mi_engine_alloc(h264mi_engine *e, size_t bytes);
int   h264mi_engine_free(h264mi_engine *e, void *p);
int   h264mi_engine_copy_h2d(h264mi_engine *e, void *dst, const void *src, size_t bytes);
/* HIP device ordinal a device pointer lives on, -1 for host / unknown memory */
int   h264mi_pointer_device(const void *p);

#ifdef __cplusplus
}
#endif

#endif
