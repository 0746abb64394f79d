/* The descriptor rules of the device-tensor exports (include/h264mi.h), stated
 * once for the engine (hip/exports.hip) and the H264SwDec calls (host/api.c).
 * Each descriptor's rules come in two parts, because api.c refuses the first
 * before it looks for headers and the second before it takes a picture:
 *   *_fixed_ok    what does not depend on the picture (element type, channels,
 *                 planes, filter, output size);
 *   *_window_ok   the window against a picture size (call it after *_fixed_ok).
 * An export accepts a descriptor that passes both.  The mode of a tensor
 * descriptor is not judged here: the engine-level calls refuse
 * H264MI_TENSOR_COLOUR_STREAM, the H264SwDec calls resolve it. */
#ifndef H264MI_EXPORT_DESC_H
#define H264MI_EXPORT_DESC_H

#include <stddef.h>
#include <stdint.h>
#include "../../../include/h264mi.h"

#define H264MI_RESIZE_MAX_DIM 16384     /* ow, oh, cw, ch of a resized export (resize.hip's RESIZE_MAX_DIM) */

#ifdef __cplusplus
#define EXPORT_CONSTEXPR constexpr      /* exports.hip checks it against the kernels' tensor_elem_size */
#else
#define EXPORT_CONSTEXPR
#endif

static inline EXPORT_CONSTEXPR size_t export_elem_size(int dtype)
{
    return dtype == H264MI_TENSOR_U8 ? 1 : dtype == H264MI_TENSOR_F32 ? 4 : 2;
}

/* the element types of the MB side-information and residual exports: a float or int16 */
static inline int export_dtype_field(int dtype)
{
    return dtype == H264MI_TENSOR_F16 || dtype == H264MI_TENSOR_BF16 || dtype == H264MI_TENSOR_F32 ||
           dtype == H264MI_TENSOR_I16;
}

/* d_out, and the distance between two pictures, are multiples of the element size */
static inline int export_aligned(const void *d_out, size_t out_stride, size_t es)
{
    return !(((size_t)(uintptr_t)d_out | out_stride) & (es - 1));
}

/* a window in luma samples of the MB-aligned picture; even: x, y, cw and ch are all even */
static inline int export_luma_window_ok(int x, int y, int cw, int ch, int w_mbs, int h_mbs, int even)
{
    return x >= 0 && y >= 0 && cw >= 1 && ch >= 1 && cw <= 16 * w_mbs - x && ch <= 16 * h_mbs - y &&
           (!even || !((x | y | cw | ch) & 1));
}

/* a channel list: 1..max ids, each below n */
static inline int export_ids_ok(const int *id, int count, int max, int n)
{
    if (count < 1 || count > max) return 0;
    for (int c = 0; c < count; c++)
        if (id[c] < 0 || id[c] >= n) return 0;
    return 1;
}

/* h264mi_tensor_desc: a pixel window is even and lies inside width x height */
static inline int tensor_desc_fixed_ok(const h264mi_tensor_desc *t)
{
    return t->dtype >= H264MI_TENSOR_U8 && t->dtype <= H264MI_TENSOR_F32;
}

static inline int tensor_window_ok(const h264mi_tensor_desc *t, int width, int height)
{
    return t->x >= 0 && t->y >= 0 && t->cw > 0 && t->ch > 0 && !((t->x | t->y | t->cw | t->ch) & 1) &&
           t->cw <= width - t->x && t->ch <= height - t->y;
}

/* h264mi_tensor_resize_desc: a known filter (1 is reserved), and at most
 * resize_max_ratio source samples per output and axis -- 64 taps either way:
 * the triangle's support is one output wide each side, the bicubic's two */
static inline int resize_filter_ok(int filter)
{
    return filter == H264MI_RESIZE_TRIANGLE || filter == H264MI_RESIZE_BICUBIC;
}

static inline int resize_max_ratio(int filter)
{
    return filter == H264MI_RESIZE_BICUBIC ? 16 : 32;
}

static inline int resize_desc_fixed_ok(const h264mi_tensor_resize_desc *d)
{
    return tensor_desc_fixed_ok(&d->t) && resize_filter_ok(d->filter) && d->ow >= 1 && d->oh >= 1 &&
           d->ow <= H264MI_RESIZE_MAX_DIM && d->oh <= H264MI_RESIZE_MAX_DIM;
}

static inline int resize_window_ok(const h264mi_tensor_resize_desc *d, int width, int height)
{
    const int ratio = resize_max_ratio(d->filter);
    return tensor_window_ok(&d->t, width, height) && d->t.cw <= H264MI_RESIZE_MAX_DIM &&
           d->t.ch <= H264MI_RESIZE_MAX_DIM && d->t.cw <= ratio * d->ow && d->t.ch <= ratio * d->oh;
}

/* a list of h264mi_roi over npics pictures of width x height under d: at least
 * one box, every pic in [0, npics), every box a window resize_window_ok accepts
 * with d's (ow, oh), and d's own window reserved (all zero).  All or nothing. */
static inline int rois_ok(const h264mi_tensor_resize_desc *d, const h264mi_roi *r, int nrois, int npics, int width,
                          int height)
{
    if (nrois < 1 || !resize_desc_fixed_ok(d) || (d->t.x | d->t.y | d->t.cw | d->t.ch)) return 0;
    for (int k = 0; k < nrois; k++) {
        h264mi_tensor_resize_desc b = *d;
        b.t.x = r[k].x; b.t.y = r[k].y; b.t.cw = r[k].cw; b.t.ch = r[k].ch;
        if (r[k].pic < 0 || r[k].pic >= npics || !resize_window_ok(&b, width, height)) return 0;
    }
    return 1;
}

/* The fit of a cw x ch window into an ow x oh canvas (include/h264mi.h, DESIGN
 * 3.5l), all four at least 1: out = (rw, rh, px, py), the content's size and
 * its place in the canvas.  The major axis fills the canvas; the minor axis
 * is the nearest integer to the exact size (halves up), but at least
 * ceil(n / 32) -- 47 rows at exactly 32 : 1 would round to 1 row, 47 source
 * samples for one output -- and at least 1.  Stated here once: the exports,
 * the H264SwDec calls and h264mi_letterbox_fit all come through it. */
static inline int letterbox_minor(int64_t n_minor, int64_t n_major, int64_t m_major)
{
    const int64_t m = (2 * n_minor * m_major + n_major) / (2 * n_major), least = (n_minor + 31) / 32;
    return (int)(m > least ? (m > 1 ? m : 1) : (least > 1 ? least : 1));
}

static inline void letterbox_fit(int cw, int ch, int ow, int oh, int fit, int out[4])
{
    int rw = ow, rh = oh;
    if (fit != H264MI_FIT_STRETCH) {
        if ((int64_t)cw * oh >= (int64_t)ch * ow) rh = letterbox_minor(ch, cw, ow);
        else rw = letterbox_minor(cw, ch, oh);
    }
    out[0] = rw; out[1] = rh;
    out[2] = fit == H264MI_FIT_LETTERBOX ? (ow - rw) / 2 : 0;
    out[3] = fit == H264MI_FIT_LETTERBOX ? (oh - rh) / 2 : 0;
}

/* h264mi_tensor_fit_desc: the resize descriptor's rules with the window judged
 * against its content size, a known fit, and the reserved pad byte zero */
static inline int fit_desc_fixed_ok(const h264mi_tensor_fit_desc *d)
{
    return resize_desc_fixed_ok(&d->r) && d->fit >= H264MI_FIT_STRETCH && d->fit <= H264MI_FIT_LETTERBOX_TOPLEFT &&
           d->pad[3] == 0;
}

/* (after fit_desc_fixed_ok) place, not NULL: the window's (rw, rh, px, py) */
static inline int fit_window_ok(const h264mi_tensor_fit_desc *d, int width, int height, int place[4])
{
    const h264mi_tensor_desc *t = &d->r.t;
    const int ratio = resize_max_ratio(d->r.filter);
    int f[4];
    if (!tensor_window_ok(t, width, height) || t->cw > H264MI_RESIZE_MAX_DIM || t->ch > H264MI_RESIZE_MAX_DIM) return 0;
    letterbox_fit(t->cw, t->ch, d->r.ow, d->r.oh, d->fit, f);
    if (place) { place[0] = f[0]; place[1] = f[1]; place[2] = f[2]; place[3] = f[3]; }
    /* (a content larger than the canvas: only behind a major axis beyond 32 : 1; letterbox_fit is one function
     * for both filters, so a bicubic content between 16 : 1 and 32 : 1 on an axis is refused here) */
    return f[0] <= d->r.ow && f[1] <= d->r.oh && t->cw <= ratio * f[0] && t->ch <= ratio * f[1];
}

/* rois_ok for a fit descriptor: every box is a window fit_window_ok accepts
 * with its own fit into d's canvas.  All or nothing. */
static inline int rois_fit_ok(const h264mi_tensor_fit_desc *d, const h264mi_roi *r, int nrois, int npics, int width,
                              int height)
{
    if (nrois < 1 || !fit_desc_fixed_ok(d) || (d->r.t.x | d->r.t.y | d->r.t.cw | d->r.t.ch)) return 0;
    for (int k = 0; k < nrois; k++) {
        h264mi_tensor_fit_desc b = *d;
        b.r.t.x = r[k].x; b.r.t.y = r[k].y; b.r.t.cw = r[k].cw; b.r.t.ch = r[k].ch;
        if (r[k].pic < 0 || r[k].pic >= npics || !fit_window_ok(&b, width, height, NULL)) return 0;
    }
    return 1;
}

/* h264mi_tensor_layout_desc: a known layout over either the unresized export
 * (no size: the tensor descriptor's rules, and nothing of the fit set) or the
 * fit descriptor with its own rules (STRETCH: the resized export) */
static inline int layout_unresized(const h264mi_tensor_layout_desc *d)
{
    return d->f.r.ow == 0 && d->f.r.oh == 0;
}

static inline int layout_desc_fixed_ok(const h264mi_tensor_layout_desc *d)
{
    if (d->layout != H264MI_LAYOUT_PLANAR && d->layout != H264MI_LAYOUT_INTERLEAVED) return 0;
    if (!layout_unresized(d)) return fit_desc_fixed_ok(&d->f);
    return tensor_desc_fixed_ok(&d->f.r.t) && d->f.fit == H264MI_FIT_STRETCH && d->f.r.filter == 0 &&
           !(d->f.pad[0] | d->f.pad[1] | d->f.pad[2] | d->f.pad[3]);
}

/* (after layout_desc_fixed_ok) */
static inline int layout_window_ok(const h264mi_tensor_layout_desc *d, int width, int height)
{
    return layout_unresized(d) ? tensor_window_ok(&d->f.r.t, width, height) : fit_window_ok(&d->f, width, height, NULL);
}

/* rois_fit_ok under a layout descriptor: boxes require a size */
static inline int rois_layout_ok(const h264mi_tensor_layout_desc *d, const h264mi_roi *r, int nrois, int npics,
                                 int width, int height)
{
    return layout_desc_fixed_ok(d) && !layout_unresized(d) && rois_fit_ok(&d->f, r, nrois, npics, width, height);
}

/* h264mi_tensor_warp_desc: the tensor descriptor's rules, an output size as for
 * the resize, a known filter, border and layout, the reserved pad byte zero,
 * and no pad where the border repeats the edge.  Its window is the one the
 * taps are confined to (common/warp_geom.h): at most 16384 a side.  The
 * matrices have no rule: every int32 coefficient is legal. */
static inline int warp_desc_fixed_ok(const h264mi_tensor_warp_desc *d)
{
    return tensor_desc_fixed_ok(&d->t) && d->ow >= 1 && d->oh >= 1 && d->ow <= H264MI_RESIZE_MAX_DIM &&
           d->oh <= H264MI_RESIZE_MAX_DIM && d->filter == H264MI_WARP_BILINEAR &&
           (d->border == H264MI_WARP_BORDER_CONSTANT || d->border == H264MI_WARP_BORDER_REPLICATE) && d->pad[3] == 0 &&
           (d->border != H264MI_WARP_BORDER_REPLICATE || !(d->pad[0] | d->pad[1] | d->pad[2])) &&
           (d->layout == H264MI_LAYOUT_PLANAR || d->layout == H264MI_LAYOUT_INTERLEAVED);
}

/* (after warp_desc_fixed_ok) */
static inline int warp_window_ok(const h264mi_tensor_warp_desc *d, int width, int height)
{
    return tensor_window_ok(&d->t, width, height) && d->t.cw <= H264MI_RESIZE_MAX_DIM && d->t.ch <= H264MI_RESIZE_MAX_DIM;
}

/* a list of h264mi_warp over npics pictures: at least one, every pic in [0, npics).  All or nothing. */
static inline int warps_ok(const h264mi_warp *w, int nwarps, int npics)
{
    if (nwarps < 1) return 0;
    for (int k = 0; k < nwarps; k++)
        if (w[k].pic < 0 || w[k].pic >= npics) return 0;
    return 1;
}

/* h264mi_stats_desc: a known plane set, no unknown flag, nothing
 * reserved, and a colour id 0..3 that only RGB reads (0 otherwise; never
 * H264MI_TENSOR_COLOUR_STREAM: api.c resolves it first).  Its window has the
 * pixel exports' rules and no size cap. */
static inline int stats_desc_fixed_ok(const h264mi_stats_desc *d)
{
    return d->planes >= H264MI_STATS_Y && d->planes <= H264MI_STATS_RGB && !(d->flags & ~H264MI_STATS_HIST) &&
           d->reserved == 0 && d->colour >= 0 &&
           d->colour <= (d->planes == H264MI_STATS_RGB ? H264MI_TENSOR_COLOUR_BT709_FULL : 0);
}

static inline int stats_box_ok(int x, int y, int cw, int ch, int width, int height)
{
    return x >= 0 && y >= 0 && cw > 0 && ch > 0 && !((x | y | cw | ch) & 1) && cw <= width - x && ch <= height - y;
}

/* (after stats_desc_fixed_ok) */
static inline int stats_window_ok(const h264mi_stats_desc *d, int width, int height)
{
    return stats_box_ok(d->x, d->y, d->cw, d->ch, width, height);
}

/* a list of h264mi_roi over npics pictures under d: at least one box, every pic
 * in [0, npics), every box a window stats_window_ok accepts, and d's own
 * window reserved (all zero).  All or nothing. */
static inline int stats_rois_ok(const h264mi_stats_desc *d, const h264mi_roi *r, int nrois, int npics, int width, int height)
{
    if (nrois < 1 || !stats_desc_fixed_ok(d) || (d->x | d->y | d->cw | d->ch)) return 0;
    for (int k = 0; k < nrois; k++)
        if (r[k].pic < 0 || r[k].pic >= npics || !stats_box_ok(r[k].x, r[k].y, r[k].cw, r[k].ch, width, height)) return 0;
    return 1;
}

/* the int64 words of an item, P * L; 0 for a bad plane set or flag */
static inline size_t stats_item_words(const h264mi_stats_desc *d)
{
    if (d->planes < H264MI_STATS_Y || d->planes > H264MI_STATS_RGB || (d->flags & ~H264MI_STATS_HIST)) return 0;
    return (size_t)(d->planes == H264MI_STATS_Y ? 1 : 3) *
           (H264MI_STATS_WORDS + (d->flags & H264MI_STATS_HIST ? H264MI_STATS_BINS : 0));
}

/* h264mi_tensor_dest over items of planes x rows x cols elements
 * of es bytes: the strides an export runs with, the descriptor's zeros filled
 * in (NULL: the packed item, one item per clip) */
typedef struct { int64_t row, plane, frame; int clip; } export_dest;

static inline export_dest dest_resolve(const h264mi_tensor_dest *d, size_t es, int planes, int rows, int cols,
                                       int interleaved)
{
    export_dest o;
    const int64_t packed = (int64_t)cols * (int64_t)es * (interleaved ? planes : 1);
    o.row = d && d->row ? d->row : packed;
    o.plane = interleaved ? 0 : d && d->plane ? d->plane : (int64_t)rows * o.row;
    o.frame = d ? d->frame : 0;
    o.clip = d ? d->clip : 1;
    return o;
}

/* what the rules of include/h264mi.h say of the descriptor alone, whatever the
 * items are: no negative stride, a clip, nothing reserved, no frame stride
 * without a clip, and no plane stride under an interleaved layout.  api.c
 * refuses on these before it looks for headers. */
static inline int dest_fixed_ok(const h264mi_tensor_dest *d, int interleaved)
{
    return !d || (d->row >= 0 && d->plane >= 0 && d->frame >= 0 && d->clip >= 1 && d->reserved == 0 &&
                  (d->clip > 1 || d->frame == 0) && (!interleaved || d->plane == 0));
}

/* the rules of include/h264mi.h for nitems items out_stride apart (dest_fixed_ok
 * among them).  The levels with more than one element, sorted by stride (at
 * most four: an insertion sort), must each step over the span of those below;
 * a span that does not fit 63 bits is refused -- a row whose rows * row does
 * not, before dest_resolve multiplies them. */
static inline int dest_ok(const h264mi_tensor_dest *d, size_t es, int planes, int rows, int cols, int interleaved,
                          int nitems, size_t out_stride)
{
    if (es < 1 || planes < 1 || rows < 1 || cols < 1 || nitems < 1 || out_stride > (size_t)INT64_MAX) return 0;
    if (!dest_fixed_ok(d, interleaved) || (d && d->row > INT64_MAX / rows)) return 0;
    const export_dest r = dest_resolve(d, es, planes, rows, cols, interleaved);
    const int64_t e = (int64_t)es, packed = (int64_t)cols * e * (interleaved ? planes : 1);
    if (r.row % e || r.plane % e || r.frame % e || (int64_t)out_stride % e) return 0;
    if (r.row < packed || nitems % r.clip) return 0;
    int64_t stride[4], count[4];
    int n = 0;
    const int64_t ls[4] = {r.row, r.plane, r.frame, (int64_t)out_stride};
    const int64_t lc[4] = {rows, interleaved ? 1 : planes, r.clip, nitems / r.clip};
    for (int l = 0; l < 4; l++) {
        if (lc[l] < 2) continue;
        int k = n++;
        for (; k > 0 && stride[k - 1] > ls[l]; k--) { stride[k] = stride[k - 1]; count[k] = count[k - 1]; }
        stride[k] = ls[l]; count[k] = lc[l];
    }
    int64_t span = packed;
    for (int k = 0; k < n; k++) {
        if (stride[k] < span || stride[k] > (INT64_MAX - span) / (count[k] - 1)) return 0;
        span += (count[k] - 1) * stride[k];
    }
    return 1;
}

/* h264mi_mbinfo_desc: the window is in 4x4 blocks of a w_mbs x h_mbs picture */
static inline int mbinfo_desc_fixed_ok(const h264mi_mbinfo_desc *d)
{
    return export_ids_ok(d->ch, d->nch, H264MI_MBINFO_MAX_CH, H264MI_MBINFO_NCHANNELS) && export_dtype_field(d->dtype);
}

static inline int mbinfo_window_ok(const h264mi_mbinfo_desc *d, int w_mbs, int h_mbs)
{
    return d->bx >= 0 && d->by >= 0 && d->bw >= 1 && d->bh >= 1 && d->bw <= 4 * w_mbs - d->bx &&
           d->bh <= 4 * h_mbs - d->by;
}

/* h264mi_residual_desc: the window is in luma samples of the MB-aligned picture, even for UV */
static inline int residual_desc_fixed_ok(const h264mi_residual_desc *d)
{
    return (d->planes == H264MI_RESID_Y || d->planes == H264MI_RESID_UV || d->planes == H264MI_RESID_YUV) &&
           export_dtype_field(d->dtype);
}

static inline int residual_window_ok(const h264mi_residual_desc *d, int w_mbs, int h_mbs)
{
    return export_luma_window_ok(d->x, d->y, d->cw, d->ch, w_mbs, h_mbs, d->planes == H264MI_RESID_UV);
}

/* h264mi_accmv_desc: an origin map holds 15-bit coordinates, and the window is
 * in luma samples of the MB-aligned picture (residual_window_ok's rules for Y) */
static inline int accmv_size_ok(int w_mbs, int h_mbs)
{
    return w_mbs >= 1 && h_mbs >= 1 && w_mbs <= H264MI_ACCMV_MAX_DIM / 16 && h_mbs <= H264MI_ACCMV_MAX_DIM / 16;
}

static inline int accmv_desc_fixed_ok(const h264mi_accmv_desc *d)
{
    return export_ids_ok(d->id, d->nch, H264MI_ACCMV_MAX_CH, H264MI_ACCMV_NCHANNELS) && export_dtype_field(d->dtype);
}

static inline int accmv_window_ok(const h264mi_accmv_desc *d, int w_mbs, int h_mbs)
{
    return accmv_size_ok(w_mbs, h_mbs) && export_luma_window_ok(d->x, d->y, d->cw, d->ch, w_mbs, h_mbs, 0);
}

/* h264mi_accres_desc: planes, element type, a colour id 0..3 (never
 * H264MI_TENSOR_COLOUR_STREAM) and a policy; the window is accmv_window_ok's,
 * even for UV */
static inline int accres_desc_fixed_ok(const h264mi_accres_desc *d)
{
    return d->planes >= H264MI_ACCRES_Y && d->planes <= H264MI_ACCRES_RGB && export_dtype_field(d->dtype) &&
           d->colour >= 0 && d->colour <= H264MI_TENSOR_COLOUR_BT709_FULL &&
           (d->unanchored == H264MI_ACCRES_KEY || d->unanchored == H264MI_ACCRES_ZERO);
}

static inline int accres_window_ok(const h264mi_accres_desc *d, int w_mbs, int h_mbs)
{
    return accmv_size_ok(w_mbs, h_mbs) &&
           export_luma_window_ok(d->x, d->y, d->cw, d->ch, w_mbs, h_mbs, d->planes == H264MI_ACCRES_UV);
}

/* h264mi_accmv_resize_desc and h264mi_accres_resize_desc: the inner
 * descriptor's rules, resize_desc_*_ok's on the output size, and its bounds on
 * the source grid gw x gh -- the window, or its half-resolution grid for UV.
 * The fields are filtered by the triangle only (H264MI_RESIZE_BICUBIC is refused). */
static inline int field_resize_size_ok(int ow, int oh, int filter)
{
    return filter == H264MI_RESIZE_TRIANGLE && ow >= 1 && oh >= 1 && ow <= H264MI_RESIZE_MAX_DIM &&
           oh <= H264MI_RESIZE_MAX_DIM;
}

static inline int field_resize_grid_ok(int gw, int gh, int ow, int oh)
{
    return gw <= H264MI_RESIZE_MAX_DIM && gh <= H264MI_RESIZE_MAX_DIM && gw <= 32 * ow && gh <= 32 * oh;
}

static inline int accmv_resize_fixed_ok(const h264mi_accmv_resize_desc *d)
{
    return accmv_desc_fixed_ok(&d->f) && field_resize_size_ok(d->ow, d->oh, d->filter);
}

static inline int accmv_resize_window_ok(const h264mi_accmv_resize_desc *d, int w_mbs, int h_mbs)
{
    return accmv_window_ok(&d->f, w_mbs, h_mbs) && field_resize_grid_ok(d->f.cw, d->f.ch, d->ow, d->oh);
}

static inline int accres_resize_fixed_ok(const h264mi_accres_resize_desc *d)
{
    return accres_desc_fixed_ok(&d->f) && field_resize_size_ok(d->ow, d->oh, d->filter);
}

static inline int accres_resize_window_ok(const h264mi_accres_resize_desc *d, int w_mbs, int h_mbs)
{
    const int hs = d->f.planes == H264MI_ACCRES_UV;
    return accres_window_ok(&d->f, w_mbs, h_mbs) && field_resize_grid_ok(d->f.cw >> hs, d->f.ch >> hs, d->ow, d->oh);
}

/* An SPS's crop window in luma samples (the whole picture without cropping;
 * the offsets are in the SPS's units of 2 samples) */
typedef struct { int x, y, cw, ch; } export_window;

static inline export_window export_crop_window(int w_mbs, int h_mbs, int crop, int crop_l, int crop_r, int crop_t,
                                               int crop_b)
{
    export_window w = {0, 0, 16 * w_mbs, 16 * h_mbs};
    if (crop) {
        w.x = 2 * crop_l; w.y = 2 * crop_t;
        w.cw -= 2 * (crop_l + crop_r); w.ch -= 2 * (crop_t + crop_b);
    }
    return w;
}

/* the 4x4 blocks that cover a window of luma samples, as (bx, by, bw, bh) */
static inline export_window export_window_blocks(export_window w)
{
    export_window b = {w.x >> 2, w.y >> 2, 0, 0};
    b.cw = ((w.x + w.cw + 3) >> 2) - b.x;
    b.ch = ((w.y + w.ch + 3) >> 2) - b.y;
    return b;
}

#endif
