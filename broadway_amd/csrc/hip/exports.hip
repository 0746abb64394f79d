// h264mi engine, export side: the entry points of every export kernel (RGBA,
// crop, tensors, statistics, MB fields, residual, accumulated motion and residual), the
// engine-level exports over them, and what an engine retains for them
// (engine_priv.h engine_exports).  Its own translation unit and code object:
// it never includes recon_kernels.hip, so no change here reaches k_prep,
// k_wgpp or k_conceal, and the core (engine.hip) reaches it through the three
// hooks of engine_priv.h.
#include "color.hip"
#include "crop.hip"
#include "tensor.hip"
#include "resize.hip"
#include "warp.hip"
#include "stats.hip"
#include "field_store.h"
#include "mbinfo.hip"
#include "residual.hip"
#include "accmv.hip"
#include "accres.hip"
#include "field_resize.hip"

#include <stdio.h>
#include <vector>
#include <stdlib.h>
#include <string.h>
#include "../../../include/h264mi.h"
#include "../common/export_desc.h"
#include "../common/warp_geom.h"
#include "engine_priv.h"

// record retention (h264mi_engine_keep_records): the uploaded batch's records,
// picture i at d_rec + i * nmbs, into the kept batches of the slots they were
// reconstructed into -- one device-to-device copy each on the engine's stream,
// behind the upload and the launch reading them and ahead of the next upload
static int keep_batch(h264mi_engine *e, int npics, const int *stream, const int *cur_slot)
{
    for (int i = 0; i < npics; i++)
        HIPCHECK(hipMemcpyAsync(e->exp.d_keep + ((size_t)stream[i] * e->nslots + cur_slot[i]) * e->nmbs,
                                e->d_rec + (size_t)i * e->nmbs, sizeof(MbRec) * e->nmbs, hipMemcpyDeviceToDevice, e->st));
    return 0;
}

// origin-map retention (h264mi_engine_keep_accmv): one k_accmv_step launch per
// ACCMV_STEP_PICS pictures of the uploaded batch, behind the launch that
// reconstructs them and ahead of the next upload, reading d_rec in place.
// Picture i's host records recs[i] say whether it is a key picture (no MBT_INTER
// / MBT_SKIP record): that bumps its stream's key serial.  A slot's map counts
// iff it was written under the stream's current serial; the slot being written
// counts as none (a picture does not reference its own slot).
static size_t acc_words(const h264mi_engine *e) { return (size_t)e->nmbs * 256; }
static int accmv_clear(h264mi_engine *e, size_t first, size_t n);

// Key-picture retention (h264mi_engine_keep_accres): the samples of `slot`,
// which holds the stream's current key picture (serial s = acc_key[stream]),
// into the stream's entry s % akey_n, behind everything queued on the engine's
// stream so far -- the launch that reconstructs the slot is.  An export that
// reads the entry's previous picture (serial s - akey_n) runs on the same
// stream (export_ordered), so this copy waits for it as a decode into a slot
// waits for the slot's export.
static int accres_copy_key(h264mi_engine *e, int stream, int slot)
{
    const unsigned long long s = e->exp.acc_key[stream];
    const size_t entry = (size_t)stream * e->exp.akey_n + (size_t)(s % (unsigned)e->exp.akey_n);
    HIPCHECK(hipMemcpyAsync(e->exp.d_akey + entry * e->frame_bytes,
                            e->d_frames + e->frame_bytes * ((size_t)stream * e->nslots + slot), e->frame_bytes,
                            hipMemcpyDeviceToDevice, e->st));
    e->exp.akey_tag[entry] = s;
    return 0;
}

// a picture that is no key picture and is decoded into the slot of its stream's
// current key: the second pass of a concealment (host/conceal.c: the concealed
// MBs are zero-vector skip records that name the slot itself, which no other
// picture does) reconstructs the key picture again, now filtered; any other
// picture replaces it
static bool accres_second_pass(const h264mi_engine *e, const MbRec *r, int slot)
{
    for (int m = 0; m < e->nmbs; m++)
        if (r[m].type <= MBT_SKIP && r[m].ref[0] == slot) return true;
    return false;
}

static int accmv_batch(h264mi_engine *e, int npics, const int *stream, const int *cur_slot, const void *const *recs)
{
    accmv_step_args a;
    a.rec = (const uint8_t *)e->d_rec;
    a.w_mbs = e->w; a.W = 16 * e->w; a.H = 16 * e->h; a.nslots = e->nslots;
    for (int k0 = 0; k0 < npics; k0 += ACCMV_STEP_PICS) {
        const int n = npics - k0 < ACCMV_STEP_PICS ? npics - k0 : ACCMV_STEP_PICS;
        memset(a.ref, 0, sizeof(a.ref));
        for (int k = 0; k < ACCMV_STEP_PICS; k++) {
            const int i = k0 + (k < n ? k : 0);
            const size_t b = (size_t)stream[i] * e->nslots;
            a.rec_off[k] = (unsigned long long)i * e->nmbs * sizeof(MbRec);
            a.out[k] = e->exp.d_acc + (b + cur_slot[i]) * acc_words(e);
            a.mode[k] = ACCMV_STEP;
            if (k >= n) continue;
            const MbRec *r = (const MbRec *)recs[i];
            bool key = true;
            for (int m = 0; m < e->nmbs && key; m++) key = r[m].type > MBT_SKIP;
            if (key) {
                e->exp.acc_key[stream[i]]++;
                a.mode[k] = ACCMV_KEY;
            } else {
                for (int s = 0; s < e->nslots; s++)
                    if (s != cur_slot[i] && e->exp.acc_key[stream[i]] && e->exp.acc_ser[b + s] == e->exp.acc_key[stream[i]])
                        a.ref[k][s] = e->exp.d_acc + (b + s) * acc_words(e);
            }
            e->exp.acc_ser[b + cur_slot[i]] = e->exp.acc_key[stream[i]];
            if (!e->exp.d_akey) continue;
            // (a later picture of this batch into the same slot leaves nothing to copy after the launch)
            bool last = true;
            for (int j = i + 1; j < npics && last; j++) last = stream[j] != stream[i] || cur_slot[j] != cur_slot[i];
            if (key) {
                e->exp.akey_slot[stream[i]] = last ? cur_slot[i] : -1;
                if (last && accres_copy_key(e, stream[i], cur_slot[i])) return -1;
            } else if (e->exp.akey_slot[stream[i]] == cur_slot[i]) {
                if (last && accres_second_pass(e, r, cur_slot[i])) {
                    if (accres_copy_key(e, stream[i], cur_slot[i])) return -1;
                } else {
                    e->exp.akey_slot[stream[i]] = -1;
                }
            }
        }
        accmv_step_launch(n, e->st, a);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// coefficient retention (h264mi_engine_keep_coefs): a kept batch holds the
// worst case of every MB -- 16 luma, 8 chroma AC, 1 luma DC and 2 chroma DC
// blocks (I_PCM's 12 fit)
#define KEEP_COEF_MB 27
static size_t keepc_cap(const h264mi_engine *e) { return (size_t)KEEP_COEF_MB * e->nmbs; }

// the same for the uploaded pool: picture i's ncoef[i] blocks, which follow
// those of the pictures before it in d_coef, to the start of its slot's kept
// batch (the records are picture-relative: the kept base is 0).  A picture
// with more blocks than a batch holds is not kept and its slot exports zeros.
static int keep_coef_batch(h264mi_engine *e, int npics, const int *stream, const int *cur_slot, const uint32_t *ncoef)
{
    size_t cbase = 0;
    for (int i = 0; i < npics; cbase += ncoef[i++]) {
        const size_t k = (size_t)stream[i] * e->nslots + cur_slot[i];
        e->exp.keepc_ok[k] = ncoef[i] <= keepc_cap(e);
        if (e->exp.keepc_ok[k] && ncoef[i])
            HIPCHECK(hipMemcpyAsync(e->exp.d_keepc + k * keepc_cap(e) * 16, e->d_coef + cbase * 16, (size_t)ncoef[i] * 32,
                                    hipMemcpyDeviceToDevice, e->st));
    }
    return 0;
}

// what is kept of the uploaded batch, queued behind its launch
int engine_exports_retain(h264mi_engine *e, int npics, const int *stream, const int *cur_slot, const void *const *recs,
                          const uint32_t *ncoef)
{
    if (e->exp.d_acc && accmv_batch(e, npics, stream, cur_slot, recs)) return -1;
    if (e->exp.d_keep && keep_batch(e, npics, stream, cur_slot)) return -1;
    return e->exp.d_keepc ? keep_coef_batch(e, npics, stream, cur_slot, ncoef) : 0;
}

// the slot's samples changed after its reconstruction: a key picture's copy is taken again
int engine_exports_slot_changed(h264mi_engine *e, int stream, int slot)
{
    return e->exp.d_akey && e->exp.akey_slot[stream] == slot ? accres_copy_key(e, stream, slot) : 0;
}

void engine_exports_free(h264mi_engine *e)
{
    (void)hipFree(e->exp.d_rgba);
    (void)hipFree(e->exp.d_keep);
    (void)hipFree(e->exp.d_keepc);
    free(e->exp.keepc_ok);
    (void)hipFree(e->exp.d_acc);
    free(e->exp.acc_key);
    free(e->exp.acc_ser);
    (void)hipFree(e->exp.d_akey);
    free(e->exp.akey_tag);
    free(e->exp.akey_slot);
    if (e->exp.ev_exp_in) (void)hipEventDestroy(e->exp.ev_exp_in);
    if (e->exp.ev_exp_out) (void)hipEventDestroy(e->exp.ev_exp_out);
}

// I420 -> RGBA (DecoderPost.js `rgb: true`, color.hip) for `npics` pictures
// of width x height pixels at in + k * in_stride -> out + k * out_stride,
// device pointers, on `stream` (NULL: the null stream); asynchronous
extern "C" int h264mi_yuv2rgba_device_pitch(const void *d_i420, void *d_rgba, int width, int height, int cpitch,
                                            int npics, size_t in_stride, size_t out_stride, void *stream)
{
    if (!d_i420 || !d_rgba || width <= 0 || height <= 0 || (width & 15) || (height & 15) || npics < 1 ||
        cpitch < width / 2)
        return -1;
    const int nblk = ((height >> 1) * (width >> 2) + 127) >> 7;
    hipLaunchKernelGGL(k_yuv2rgba, dim3(nblk, npics), dim3(64), 0, (hipStream_t)stream,
                       (const uint8_t *)d_i420, (uint8_t *)d_rgba, width, height, cpitch, in_stride, out_stride);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int h264mi_yuv2rgba_device(const void *d_i420, void *d_rgba, int width, int height, int npics,
                                      size_t in_stride, size_t out_stride, void *stream)
{
    return h264mi_yuv2rgba_device_pitch(d_i420, d_rgba, width, height, width / 2, npics, in_stride, out_stride, stream);
}

extern "C" int h264mi_engine_read_rgba(h264mi_engine *e, int stream, int slot, uint8_t *dst)
{
    if (!e || stream < 0 || stream >= e->nstreams || slot < 0 || slot >= e->nslots) return -1;
    const size_t bytes = (size_t)e->nmbs * 256 * 4;
    if (!e->exp.d_rgba) HIPCHECK(hipMalloc(&e->exp.d_rgba, bytes));
    if (h264mi_yuv2rgba_device_pitch(e->d_frames + e->frame_bytes * ((size_t)stream * e->nslots + slot), e->exp.d_rgba,
                                     e->w * 16, e->h * 16, e->cpitch, 1, 0, 0, e->st))
        return -1;
    HIPCHECK(hipMemcpyAsync(dst, e->exp.d_rgba, bytes, hipMemcpyDeviceToHost, e->st));
    HIPCHECK(hipStreamSynchronize(e->st));
    return 0;
}

// The crop window (x, y, cw, ch; all even, inside the picture) of `npics`
// pictures of width x height pixels, chroma rows cpitch bytes apart, at
// d_in + k * in_stride -> packed at d_out + k * out_stride: I420 in the layout
// of the reference testbench's CropPicture, or RGBA (crop.hip); device
// pointers, asynchronous on `stream`.  RGBA output is 8-byte aligned.
// -1 (nothing launched) on a bad argument.
extern "C" int h264mi_crop_device_pitch(const void *d_in, void *d_out, int width, int height, int cpitch, int x, int y,
                                        int cw, int ch, int rgba, int npics, size_t in_stride, size_t out_stride,
                                        void *stream)
{
    if (!d_in || !d_out || width <= 0 || height <= 0 || ((width | height) & 1) || npics < 1 || cpitch < width / 2 ||
        x < 0 || y < 0 || cw <= 0 || ch <= 0 || ((x | y | cw | ch) & 1) || cw > width - x || ch > height - y)
        return -1;
    const uint8_t *in = (const uint8_t *)d_in;
    uint8_t *out = (uint8_t *)d_out;
    if (rgba) {
        const size_t al = (size_t)(uintptr_t)out | (npics > 1 ? out_stride : 0);
        if (al & 7) return -1;
        const int nblk = ((ch >> 1) * ((cw + 3) >> 2) + 127) >> 7;
        if (!(cw & 3) && !(al & 15))
            hipLaunchKernelGGL(k_crop_rgba<true>, dim3(nblk, npics), dim3(64), 0, (hipStream_t)stream, in, out, width,
                               height, cpitch, x, y, cw, ch, in_stride, out_stride);
        else
            hipLaunchKernelGGL(k_crop_rgba<false>, dim3(nblk, npics), dim3(64), 0, (hipStream_t)stream, in, out, width,
                               height, cpitch, x, y, cw, ch, in_stride, out_stride);
    } else {
        // the most chunks the three planes can cover, whatever the output's alignment
        const int ny = cw * ch, nc = (cw >> 1) * (ch >> 1);
        const int chunks = ((ny + 30) >> 4) + 2 * ((nc + 30) >> 4);
        hipLaunchKernelGGL(k_crop_i420, dim3((chunks + 127) >> 7, npics), dim3(64), 0, (hipStream_t)stream, in, out,
                           width, height, cpitch, x, y, cw, ch, in_stride, out_stride);
    }
    HIPCHECK(hipGetLastError());
    return 0;
}

// D2H of the crop window of a slot, packed I420 or RGBA (h264mi_crop_device_pitch
// into a staging buffer, one contiguous copy); syncs the engine first
extern "C" int h264mi_engine_read_crop(h264mi_engine *e, int stream, int slot, int x, int y, int cw, int ch, int rgba,
                                       uint8_t *dst)
{
    if (!e || !dst || stream < 0 || stream >= e->nstreams || slot < 0 || slot >= e->nslots) return -1;
    const int width = e->w * 16, height = e->h * 16;
    if (x < 0 || y < 0 || cw <= 0 || ch <= 0 || ((x | y | cw | ch) & 1) || cw > width - x || ch > height - y) return -1;
    if (h264mi_engine_sync(e)) return -1;
    const uint8_t *src = e->d_frames + e->frame_bytes * ((size_t)stream * e->nslots + slot);
    const size_t bytes = rgba ? (size_t)cw * ch * 4 : (size_t)cw * ch * 3 / 2;
    if (!e->exp.d_rgba) HIPCHECK(hipMalloc(&e->exp.d_rgba, (size_t)e->nmbs * 256 * 4));
    if (h264mi_crop_device_pitch(src, e->exp.d_rgba, width, height, e->cpitch, x, y, cw, ch, rgba, 1, 0, 0, e->st)) return -1;
    HIPCHECK(hipMemcpyAsync(dst, e->exp.d_rgba, bytes, hipMemcpyDeviceToHost, e->st));
    HIPCHECK(hipStreamSynchronize(e->st));
    return 0;
}

// a mode the engine-level exports accept: RGB with a colour id 0..3 (bits 12
// and 13 mean nothing without STREAM, which needs a stream: refused) or GRAY
// with no colour bits, and no bit from 14 up
static bool tensor_mode_ok(int mode)
{
    if (mode & ~0x3FFF) return false;
    if (H264MI_TENSOR_LAYOUT(mode) == H264MI_TENSOR_GRAY) return mode == H264MI_TENSOR_GRAY;
    return H264MI_TENSOR_LAYOUT(mode) == H264MI_TENSOR_RGB && H264MI_TENSOR_COLOUR(mode) < TENSOR_COLOUR_SETS;
}

// a window / mode / dtype a tensor export accepts (the window rules are
// h264mi_crop_device_pitch's)
static bool tensor_desc_ok(const h264mi_tensor_desc *t, int width, int height)
{
    return t && tensor_mode_ok(t->mode) && tensor_desc_fixed_ok(t) && tensor_window_ok(t, width, height);
}

extern "C" int h264mi_tensor_colour_coeffs(int id, int out[6])
{
    if (id < 0 || id >= TENSOR_COLOUR_SETS || !out) return -1;
    const colour_set &c = tensor_colour_sets[id];
    out[0] = c.ky; out[1] = c.k0; out[2] = c.crv; out[3] = c.cgu; out[4] = c.cgv; out[5] = c.cbu;
    return 0;
}

// a resize descriptor h264mi_tensor_resize_device_pitch accepts
static bool resize_desc_ok(const h264mi_tensor_resize_desc *d, int width, int height)
{
    return d && tensor_mode_ok(d->t.mode) && resize_desc_fixed_ok(d) && resize_window_ok(d, width, height);
}

// a field descriptor h264mi_mbinfo_device accepts on a w_mbs x h_mbs picture
static bool mbinfo_desc_ok(const h264mi_mbinfo_desc *d, int w_mbs, int h_mbs)
{
    return d && mbinfo_desc_fixed_ok(d) && mbinfo_window_ok(d, w_mbs, h_mbs);
}

// a residual descriptor h264mi_residual_device accepts on a w_mbs x h_mbs picture
static bool residual_desc_ok(const h264mi_residual_desc *d, int w_mbs, int h_mbs)
{
    return d && residual_desc_fixed_ok(d) && residual_window_ok(d, w_mbs, h_mbs);
}

#define EXPORT_MAX_PICS TENSOR_MAX_PICS
static_assert(MBINFO_MAX_PICS == EXPORT_MAX_PICS && RESID_MAX_PICS == EXPORT_MAX_PICS,
              "every export kernel takes the same number of pictures per launch");
static_assert(H264MI_RESIZE_MAX_DIM == RESIZE_MAX_DIM, "common/export_desc.h and resize.hip name the same bound");
static_assert(export_elem_size(H264MI_TENSOR_U8) == tensor_elem_size(TENSOR_U8) &&
                  export_elem_size(H264MI_TENSOR_F16) == tensor_elem_size(TENSOR_F16) &&
                  export_elem_size(H264MI_TENSOR_BF16) == tensor_elem_size(TENSOR_BF16) &&
                  export_elem_size(H264MI_TENSOR_F32) == tensor_elem_size(TENSOR_F32) &&
                  export_elem_size(H264MI_TENSOR_I16) == tensor_elem_size(TENSOR_I16),
              "common/export_desc.h and tensor.hip give the element types the same sizes");

// the kernels may store 16 bytes at a time: every row of row_bytes bytes of
// every picture (out_stride apart) starts on a multiple of 16
static bool export_v16(const void *d_out, size_t out_stride, size_t row_bytes)
{
    return !(((size_t)(uintptr_t)d_out | out_stride | row_bytes) & 15);
}

// The launches of a *_device entry point over npics pictures, at most
// EXPORT_MAX_PICS each: a launch's offsets into a_off, zero-padded, and its
// first picture's address into *a_out, then launch(k0, n) for the n pictures
// from k0 on.
template <class Launch>
static int export_launches(int npics, const size_t *offsets, unsigned long long *a_off, uint8_t **a_out, void *d_out,
                           size_t out_stride, Launch launch)
{
    for (int k0 = 0; k0 < npics; k0 += EXPORT_MAX_PICS) {
        const int n = npics - k0 < EXPORT_MAX_PICS ? npics - k0 : EXPORT_MAX_PICS;
        for (int k = 0; k < EXPORT_MAX_PICS; k++) a_off[k] = k < n ? offsets[k0 + k] : 0;
        *a_out = (uint8_t *)d_out + (size_t)k0 * out_stride;
        launch(k0, n);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// The launches of a pixel export (k_tensor, k_tensor_resize, k_tensor_warp)
// over nitems items under the resolved destination `ds`: as
// export_launches, but an item is placed by the descriptor -- a.out is d_out
// for every launch and grid row k's item starts a.out_off[k] bytes behind it,
// so a launch may begin and end inside a clip.  Fills a.row and a.plane.
template <class Launch>
static int dest_launches(int nitems, const size_t *offsets, tensor_args &a, void *d_out, size_t out_stride,
                         const export_dest &ds, Launch launch)
{
    a.out = (uint8_t *)d_out;
    a.row = (size_t)ds.row;
    a.plane = (size_t)ds.plane;
    for (int k0 = 0; k0 < nitems; k0 += EXPORT_MAX_PICS) {
        const int n = nitems - k0 < EXPORT_MAX_PICS ? nitems - k0 : EXPORT_MAX_PICS;
        for (int k = 0; k < EXPORT_MAX_PICS; k++) {
            const size_t item = (size_t)(k0 + k);
            a.in_off[k] = k < n ? offsets[k0 + k] : 0;
            a.out_off[k] = k < n ? (item / (size_t)ds.clip) * out_stride + (item % (size_t)ds.clip) * (size_t)ds.frame : 0;
        }
        launch(k0, n);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// k_tensor may store 16 bytes at a time under a destination: d_out, the
// distances between clips, items, planes and rows, and the packed row
static bool dest_v16(const void *d_out, size_t out_stride, const export_dest &ds, size_t row_bytes)
{
    return export_v16(d_out, out_stride, row_bytes) && !(((size_t)ds.frame | (size_t)ds.plane | (size_t)ds.row) & 15);
}

// Both tensor exports (r != NULL: resized, t = &r->t): one check and one fill
// of what their kernels share, resize_args::t.  interleaved and dest (unresized
// only, from h264mi_tensor_dest_device_pitch): the layout -- RGB: the elements
// interleaved, a row 3 cw elements; GRAY: the same bytes either way -- and the
// destination (NULL: packed items out_stride apart), judged here, behind the
// descriptor it depends on and ahead of the launches.  The resized form is the
// single-window kernel's: planar, packed pictures out_stride apart.
static int tensor_device(const void *d_in, const size_t *in_offsets, int npics, int width, int height, int cpitch,
                         const h264mi_tensor_desc *t, const h264mi_tensor_resize_desc *r, void *d_out,
                         size_t out_stride, hipStream_t stream, bool interleaved = false,
                         const h264mi_tensor_dest *dest = NULL)
{
    static_assert(H264MI_TENSOR_RGB == TENSOR_RGB && H264MI_TENSOR_GRAY == TENSOR_GRAY &&
                      H264MI_TENSOR_U8 == TENSOR_U8 && H264MI_TENSOR_F16 == TENSOR_F16 &&
                      H264MI_TENSOR_BF16 == TENSOR_BF16 && H264MI_TENSOR_F32 == TENSOR_F32 &&
                      H264MI_TENSOR_COLOUR_BT709_FULL == TENSOR_COLOUR_SETS - 1,
                  "include/h264mi.h and tensor.hip name the same modes, element types and colour sets");
    if (!d_in || !in_offsets || !d_out || width <= 0 || height <= 0 || ((width | height) & 1) || npics < 1 ||
        cpitch < width / 2 || (r ? !resize_desc_ok(r, width, height) : !tensor_desc_ok(t, width, height)))
        return -1;
    const size_t es = export_elem_size(t->dtype);
    if (!export_aligned(d_out, out_stride, es)) return -1;
    const int layout = H264MI_TENSOR_LAYOUT(t->mode), colour = H264MI_TENSOR_COLOUR(t->mode);
    if (r && (interleaved || dest)) return -1;
    const bool hwc = interleaved && layout == H264MI_TENSOR_RGB;
    resize_args ra;
    tensor_args &a = ra.t;
    a.in = (const uint8_t *)d_in;
    a.width = width; a.height = height; a.cpitch = cpitch;
    a.x = t->x; a.y = t->y; a.cw = t->cw; a.ch = t->ch;
    for (int p = 0; p < 3; p++) { a.scale[p] = t->scale[p]; a.bias[p] = t->bias[p]; }
    a.col = tensor_colour_sets[colour];     // (set 0 runs the kernels with the reference's literals)
    if (r) { ra.ow = r->ow; ra.oh = r->oh; }
    const bool cubic = r && r->filter == H264MI_RESIZE_BICUBIC;
    if (r) {
        a.out_stride = out_stride;
        a.row = a.plane = 0;
        return export_launches(npics, in_offsets, a.in_off, &a.out, d_out, out_stride,
                               [&](int, int n) { resize_launch(layout, t->dtype, colour != 0, cubic, n, stream, ra); });
    }
    if (dest && !dest_ok(dest, es, layout == H264MI_TENSOR_RGB ? 3 : 1, t->ch, t->cw, interleaved, npics, out_stride)) return -1;
    const export_dest ds = dest_resolve(dest, es, layout == H264MI_TENSOR_RGB ? 3 : 1, t->ch, t->cw, interleaved);
    const bool v16 = dest_v16(d_out, out_stride, ds, (size_t)t->cw * es * (hwc ? 3 : 1));
    a.out_stride = 0;
    return dest_launches(npics, in_offsets, a, d_out, out_stride, ds, [&](int, int n) {
        tensor_launch(layout, t->dtype, v16, colour != 0, hwc, n, stream, a);
    });
}

// Pictures as planar tensors (tensor.hip): the window desc->(x, y, cw, ch) of
// the npics pictures of width x height pixels that start in_offsets[k] bytes
// after d_in (chroma rows cpitch bytes apart), as contiguous (planes, ch, cw)
// elements of desc->dtype at d_out + k * out_stride; device pointers,
// asynchronous on `stream`; TENSOR_MAX_PICS pictures per launch.  -1 (nothing
// launched) on a bad argument.
extern "C" int h264mi_tensor_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                          int cpitch, const h264mi_tensor_desc *desc, void *d_out, size_t out_stride,
                                          void *stream)
{
    return tensor_device(d_in, in_offsets, npics, width, height, cpitch, desc, NULL, d_out, out_stride, (hipStream_t)stream);
}

// The same pictures resized (resize.hip): the window filtered to desc->oh x
// desc->ow samples per plane, picture k's (planes, oh, ow) elements at d_out +
// k * out_stride.  1 <= ow, oh <= 16384 and, per axis, at most 32 source
// samples per output under H264MI_RESIZE_TRIANGLE, 16 under
// H264MI_RESIZE_BICUBIC (64 taps either way); the filter picks the kernel's
// instantiation, here and in every resized export below.  Stateless: the tap
// tables are made in the kernel.  -1 (nothing launched) on a bad
// argument.
extern "C" int h264mi_tensor_resize_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width,
                                                 int height, int cpitch, const h264mi_tensor_resize_desc *desc,
                                                 void *d_out, size_t out_stride, void *stream)
{
    return tensor_device(d_in, in_offsets, npics, width, height, cpitch, desc ? &desc->t : NULL, desc, d_out, out_stride,
                         (hipStream_t)stream);
}

// The resized export over a list of boxes (resize.hip k_tensor_resize with
// ROIS): box r, the window rois[r].(x, y, cw, ch) of the picture that starts
// in_offsets[rois[r].pic] bytes after d_in, filtered to desc->oh x desc->ow
// samples per plane: its (planes, oh, ow) elements at d_out + r * out_stride.
// desc->t's window is reserved (zero).  Everything is checked first (rois_ok:
// one bad box refuses the call); then one launch per EXPORT_MAX_PICS boxes,
// each with its rows' picture offsets and windows in the kernel arguments.
// rois is host memory, read here.  -1 (nothing launched) on a bad argument.
static_assert(H264MI_ROIS_MAX_PER_LAUNCH == TENSOR_MAX_PICS, "include/h264mi.h and tensor.hip name the same bound");

static bool rois_desc_ok(const h264mi_tensor_resize_desc *d, const h264mi_roi *rois, int nrois, int npics, int width,
                         int height)
{
    return d && rois && tensor_mode_ok(d->t.mode) && rois_ok(d, rois, nrois, npics, width, height);
}

// The launches of the list exports, behind their checks (the descriptor's and
// the pictures').  fit != NULL (desc = &fit->r): every box fitted into the canvas (oh, ow) by
// letterbox_fit, the rest of the canvas fit->pad; whole != NULL:
// the list is `whole` of every picture (the single-window form) and rois is unused;
// hwc (RGB, fit != NULL, from h264mi_tensor_layout_device_pitch): the elements interleaved
static int rois_device(const void *d_in, const size_t *in_offsets, int npics, int width, int height, int cpitch,
                       const h264mi_tensor_resize_desc *desc, const h264mi_tensor_fit_desc *fit,
                       const h264mi_tensor_desc *whole, const h264mi_roi *rois, int nrois, void *d_out,
                       size_t out_stride, void *stream, bool hwc = false, const h264mi_tensor_dest *dest = NULL,
                       bool interleaved = false)
{
    const h264mi_tensor_desc *t = &desc->t;
    if (hwc && (!fit || H264MI_TENSOR_LAYOUT(t->mode) != H264MI_TENSOR_RGB)) return -1;
    // (d_out is checked here too: a list is one lookup, and a host address would fault every launch of it)
    if (!export_aligned(d_out, out_stride, export_elem_size(t->dtype)) || h264mi_pointer_device(d_out) < 0) return -1;
    const int layout = H264MI_TENSOR_LAYOUT(t->mode), colour = H264MI_TENSOR_COLOUR(t->mode);
    const int planes = layout == H264MI_TENSOR_RGB ? 3 : 1;
    if (dest && !dest_ok(dest, export_elem_size(t->dtype), planes, desc->oh, desc->ow, interleaved || hwc, nrois, out_stride))
        return -1;
    const export_dest ds = dest_resolve(dest, export_elem_size(t->dtype), planes, desc->oh, desc->ow, interleaved || hwc);
    fit_args fa;
    rois_args &ra = fa;
    tensor_args &a = ra.r.t;
    a.in = (const uint8_t *)d_in;
    a.width = width; a.height = height; a.cpitch = cpitch;
    a.x = a.y = a.cw = a.ch = 0;
    a.out_stride = 0;
    for (int p = 0; p < 3; p++) { a.scale[p] = t->scale[p]; a.bias[p] = t->bias[p]; }
    a.col = tensor_colour_sets[colour];
    ra.r.ow = desc->ow; ra.r.oh = desc->oh;
    const bool cubic = desc->filter == H264MI_RESIZE_BICUBIC;
    if (fit)
        for (int p = 0; p < 3; p++) fa.pad[p] = fit->pad[p];
    std::vector<size_t> off((size_t)nrois);
    for (int r = 0; r < nrois; r++) off[r] = in_offsets[whole ? r : rois[r].pic];
    return dest_launches(nrois, off.data(), a, d_out, out_stride, ds, [&](int r0, int n) {
        for (int r = 0; r < EXPORT_MAX_PICS; r++) {
            const h264mi_roi w = {0, t->x, t->y, t->cw, t->ch};
            const h264mi_roi &b = whole ? w : rois[r0 + (r < n ? r : 0)];
            ra.win[r][0] = b.x; ra.win[r][1] = b.y; ra.win[r][2] = b.cw; ra.win[r][3] = b.ch;
            if (fit) {
                int f[4];
                letterbox_fit(b.cw, b.ch, desc->ow, desc->oh, fit->fit, f);
                fa.place[r][0] = f[2]; fa.place[r][1] = f[3]; fa.place[r][2] = f[0]; fa.place[r][3] = f[1];
            }
        }
        if (hwc) fit_hwc_launch(t->dtype, colour != 0, cubic, n, (hipStream_t)stream, fa);
        else if (fit) fit_launch(layout, t->dtype, colour != 0, cubic, n, (hipStream_t)stream, fa);
        else rois_launch(layout, t->dtype, colour != 0, cubic, n, (hipStream_t)stream, ra);
    });
}

// what every stateless tensor export asks of its pictures
static bool tensor_pics_ok(const void *d_in, const size_t *in_offsets, int npics, int width, int height, int cpitch,
                           const void *d_out)
{
    return d_in && in_offsets && d_out && width > 0 && height > 0 && !((width | height) & 1) && npics >= 1 &&
           cpitch >= width / 2;
}

extern "C" int h264mi_tensor_rois_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width,
                                               int height, int cpitch, const h264mi_tensor_resize_desc *desc,
                                               const h264mi_roi *rois, int nrois, void *d_out, size_t out_stride,
                                               void *stream)
{
    if (!tensor_pics_ok(d_in, in_offsets, npics, width, height, cpitch, d_out) ||
        !rois_desc_ok(desc, rois, nrois, npics, width, height))
        return -1;
    return rois_device(d_in, in_offsets, npics, width, height, cpitch, desc, NULL, NULL, rois, nrois, d_out, out_stride,
                       stream);
}

// The letterboxed exports (include/h264mi.h): picture k's window
// desc->r.t, or box r of a list as above, scaled with its aspect ratio kept
// into the canvas desc->r.oh x desc->r.ow -- the content (rw, rh) at (px, py)
// from letterbox_fit, resolved here per row and handed to the kernel --, the
// rest of the canvas the element of desc->pad.  Both are the table form of the
// kernel: the single-window call's table has one row per picture.  -1 (nothing
// launched) on a bad argument.
extern "C" int h264mi_letterbox_fit(int cw, int ch, int ow, int oh, int fit, int out[4])
{
    if (!out || cw < 1 || ch < 1 || ow < 1 || oh < 1 || cw > H264MI_RESIZE_MAX_DIM || ch > H264MI_RESIZE_MAX_DIM ||
        ow > H264MI_RESIZE_MAX_DIM || oh > H264MI_RESIZE_MAX_DIM || fit < H264MI_FIT_STRETCH ||
        fit > H264MI_FIT_LETTERBOX_TOPLEFT)
        return -1;
    letterbox_fit(cw, ch, ow, oh, fit, out);
    return 0;
}

// a fit descriptor h264mi_tensor_fit_device_pitch accepts
static bool fit_desc_ok(const h264mi_tensor_fit_desc *d, int width, int height)
{
    return d && tensor_mode_ok(d->r.t.mode) && fit_desc_fixed_ok(d) && fit_window_ok(d, width, height, NULL);
}

static bool rois_fit_desc_ok(const h264mi_tensor_fit_desc *d, const h264mi_roi *rois, int nrois, int npics, int width,
                             int height)
{
    return d && rois && tensor_mode_ok(d->r.t.mode) && rois_fit_ok(d, rois, nrois, npics, width, height);
}

extern "C" int h264mi_tensor_fit_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width,
                                              int height, int cpitch, const h264mi_tensor_fit_desc *desc, void *d_out,
                                              size_t out_stride, void *stream)
{
    if (!tensor_pics_ok(d_in, in_offsets, npics, width, height, cpitch, d_out) || !fit_desc_ok(desc, width, height))
        return -1;
    return rois_device(d_in, in_offsets, npics, width, height, cpitch, &desc->r, desc, &desc->r.t, NULL, npics, d_out,
                       out_stride, stream);
}

extern "C" int h264mi_tensor_rois_fit_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width,
                                                   int height, int cpitch, const h264mi_tensor_fit_desc *desc,
                                                   const h264mi_roi *rois, int nrois, void *d_out, size_t out_stride,
                                                   void *stream)
{
    if (!tensor_pics_ok(d_in, in_offsets, npics, width, height, cpitch, d_out) ||
        !rois_fit_desc_ok(desc, rois, nrois, npics, width, height))
        return -1;
    return rois_device(d_in, in_offsets, npics, width, height, cpitch, &desc->r, desc, NULL, rois, nrois, d_out,
                       out_stride, stream);
}

// The four pixel exports under a layout descriptor (include/h264mi.h, DESIGN
// §3.5m): one check (common/export_desc.h), then the path of the call it
// mirrors.  PLANAR and GRAY are that call; INTERLEAVED RGB is tensor_device's
// unresized launch with its interleaved kernels, or -- every resized form, a
// stretch included -- the table form of the fit kernel with interleaved stores.
// rois == NULL (then nrois == 0): desc's window of every picture.
static bool layout_desc_ok(const h264mi_tensor_layout_desc *d, const h264mi_roi *rois, int nrois, int npics, int width,
                           int height)
{
    if (!d || !tensor_mode_ok(d->f.r.t.mode) || (rois ? nrois < 1 : nrois != 0)) return false;
    if (rois) return rois_layout_ok(d, rois, nrois, npics, width, height);
    return layout_desc_fixed_ok(d) && layout_window_ok(d, width, height);
}

//  ... into a strided destination: dest (NULL: packed items
// out_stride apart, the layout call) is judged by dest_ok with the call's items
// where the launches are made, behind every other check and ahead of the first.
extern "C" int h264mi_tensor_dest_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width,
                                               int height, int cpitch, const h264mi_tensor_layout_desc *desc,
                                               const h264mi_roi *rois, int nrois, const h264mi_tensor_dest *dest,
                                               void *d_out, size_t out_stride, void *stream)
{
    if (!tensor_pics_ok(d_in, in_offsets, npics, width, height, cpitch, d_out) ||
        !layout_desc_ok(desc, rois, nrois, npics, width, height))
        return -1;
    const h264mi_tensor_fit_desc *f = &desc->f;
    const bool il = desc->layout == H264MI_LAYOUT_INTERLEAVED;
    const bool hwc = il && H264MI_TENSOR_LAYOUT(f->r.t.mode) == H264MI_TENSOR_RGB;
    if (layout_unresized(desc))
        return tensor_device(d_in, in_offsets, npics, width, height, cpitch, &f->r.t, NULL, d_out, out_stride,
                             (hipStream_t)stream, il, dest);
    const bool stretch = f->fit == H264MI_FIT_STRETCH;
    // (a stretched single window into a destination runs as a table, one row per picture: the strides are the table forms')
    if (!rois && stretch && !hwc && !dest)
        return tensor_device(d_in, in_offsets, npics, width, height, cpitch, &f->r.t, &f->r, d_out, out_stride,
                             (hipStream_t)stream);
    return rois_device(d_in, in_offsets, npics, width, height, cpitch, &f->r, stretch && !hwc ? NULL : f,
                       rois ? NULL : &f->r.t, rois, rois ? nrois : npics, d_out, out_stride, stream, hwc, dest, il);
}

extern "C" int h264mi_tensor_layout_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width,
                                                 int height, int cpitch, const h264mi_tensor_layout_desc *desc,
                                                 const h264mi_roi *rois, int nrois, void *d_out, size_t out_stride,
                                                 void *stream)
{
    return h264mi_tensor_dest_device_pitch(d_in, in_offsets, npics, width, height, cpitch, desc, rois, nrois, NULL, d_out,
                                           out_stride, stream);
}

// The affine-warped export (warp.hip, include/h264mi.h): warp r,
// the matrix warps[r].m over the window desc->t of the picture that starts
// in_offsets[warps[r].pic] bytes after d_in: its (planes, oh, ow) elements at
// d_out + r * out_stride, interleaved with desc->layout (RGB).  Everything is
// checked first (common/export_desc.h: one bad warp refuses the call; every
// matrix is legal, the taps stay in the window by common/warp_geom.h); then one
// launch per EXPORT_MAX_PICS warps, each with its rows' picture offsets and
// matrices in the kernel arguments.  warps is host memory, read here.  -1
// (nothing launched) on a bad argument.
static_assert(H264MI_WARPS_MAX_PER_LAUNCH == TENSOR_MAX_PICS, "include/h264mi.h and tensor.hip name the same bound");

static bool warps_desc_ok(const h264mi_tensor_warp_desc *d, const h264mi_warp *warps, int nwarps, int npics, int width,
                          int height)
{
    return d && warps && tensor_mode_ok(d->t.mode) && warp_desc_fixed_ok(d) && warp_window_ok(d, width, height) &&
           warps_ok(warps, nwarps, npics);
}

extern "C" int h264mi_tensor_warps_dest_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width,
                                                     int height, int cpitch, const h264mi_tensor_warp_desc *desc,
                                                     const h264mi_warp *warps, int nwarps, const h264mi_tensor_dest *dest,
                                                     void *d_out, size_t out_stride, void *stream)
{
    if (!tensor_pics_ok(d_in, in_offsets, npics, width, height, cpitch, d_out) ||
        !warps_desc_ok(desc, warps, nwarps, npics, width, height))
        return -1;
    const h264mi_tensor_desc *t = &desc->t;
    // (d_out is checked here too, as for the boxes: a host address would fault every launch of the list)
    if (!export_aligned(d_out, out_stride, export_elem_size(t->dtype)) || h264mi_pointer_device(d_out) < 0) return -1;
    const int layout = H264MI_TENSOR_LAYOUT(t->mode), colour = H264MI_TENSOR_COLOUR(t->mode);
    const bool il = desc->layout == H264MI_LAYOUT_INTERLEAVED, hwc = il && layout == H264MI_TENSOR_RGB;
    const int planes = layout == H264MI_TENSOR_RGB ? 3 : 1;
    if (dest && !dest_ok(dest, export_elem_size(t->dtype), planes, desc->oh, desc->ow, il, nwarps, out_stride)) return -1;
    const export_dest ds = dest_resolve(dest, export_elem_size(t->dtype), planes, desc->oh, desc->ow, il);
    warp_args wa;
    tensor_args &a = wa.t;
    a.in = (const uint8_t *)d_in;
    a.width = width; a.height = height; a.cpitch = cpitch;
    a.x = t->x; a.y = t->y; a.cw = t->cw; a.ch = t->ch;
    a.out_stride = 0;
    for (int p = 0; p < 3; p++) { a.scale[p] = t->scale[p]; a.bias[p] = t->bias[p]; wa.pad[p] = desc->pad[p]; }
    a.col = tensor_colour_sets[colour];
    wa.ow = desc->ow; wa.oh = desc->oh; wa.border = desc->border;
    std::vector<size_t> off((size_t)nwarps);
    for (int r = 0; r < nwarps; r++) off[r] = in_offsets[warps[r].pic];
    return dest_launches(nwarps, off.data(), a, d_out, out_stride, ds, [&](int r0, int n) {
        for (int r = 0; r < EXPORT_MAX_PICS; r++)
            memcpy(wa.m[r], warps[r0 + (r < n ? r : 0)].m, sizeof(wa.m[r]));
        warp_launch(layout, t->dtype, colour != 0, hwc, n, (hipStream_t)stream, wa);
    });
}

extern "C" int h264mi_tensor_warps_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width,
                                                int height, int cpitch, const h264mi_tensor_warp_desc *desc,
                                                const h264mi_warp *warps, int nwarps, void *d_out, size_t out_stride,
                                                void *stream)
{
    return h264mi_tensor_warps_dest_device_pitch(d_in, in_offsets, npics, width, height, cpitch, desc, warps, nwarps, NULL,
                                                 d_out, out_stride, stream);
}

// An export of the slots (streams[k], slots[k]), k < n, into the caller's
// device memory with no host synchronisation: the engine's stream waits for
// what `stream` (NULL: the null stream; ours is non-blocking, so that too goes
// through events) holds already -- d_out may have been recycled on it --,
// launch() queues the kernels on the engine's stream, behind every launch
// queued so far and ahead of every later one, and `stream` waits for them.
// es: the element size d_out and out_stride are multiples of.
template <class Launch>
static int export_ordered(h264mi_engine *e, int n, const int *streams, const int *slots, void *d_out, size_t out_stride,
                          size_t es, void *stream, Launch launch)
{
    for (int k = 0; k < n; k++)
        if (streams[k] < 0 || streams[k] >= e->nstreams || slots[k] < 0 || slots[k] >= e->nslots) return -1;
    if (!export_aligned(d_out, out_stride, es)) return -1;
    if (h264mi_pointer_device(d_out) != e->dev) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    if (!e->exp.ev_exp_in) HIPCHECK(hipEventCreateWithFlags(&e->exp.ev_exp_in, hipEventDisableTiming));
    if (!e->exp.ev_exp_out) HIPCHECK(hipEventCreateWithFlags(&e->exp.ev_exp_out, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(e->exp.ev_exp_in, (hipStream_t)stream));
    HIPCHECK(hipStreamWaitEvent(e->st, e->exp.ev_exp_in, 0));
    const int rc = launch();
    // (also after a failed launch: whatever reached our stream stays ordered)
    HIPCHECK(hipEventRecord(e->exp.ev_exp_out, e->st));
    HIPCHECK(hipStreamWaitEvent((hipStream_t)stream, e->exp.ev_exp_out, 0));
    return rc;
}

// the frame slots as tensors (rdesc != NULL: resized, desc = &rdesc->t)
static int engine_export(h264mi_engine *e, int n, const int *streams, const int *slots, const h264mi_tensor_desc *desc,
                         const h264mi_tensor_resize_desc *rdesc, void *d_out, size_t out_stride, void *stream)
{
    if (!e || n < 1 || !streams || !slots || !d_out) return -1;
    const int width = e->w * 16, height = e->h * 16;
    if (rdesc ? !resize_desc_ok(rdesc, width, height) : !tensor_desc_ok(desc, width, height)) return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->dtype), stream, [&] {
        std::vector<size_t> off((size_t)n);
        for (int k = 0; k < n; k++) off[k] = e->frame_bytes * ((size_t)streams[k] * e->nslots + slots[k]);
        return tensor_device(e->d_frames, off.data(), n, width, height, e->cpitch, desc, rdesc, d_out, out_stride, e->st);
    });
}

extern "C" int h264mi_engine_export_tensor(h264mi_engine *e, int n, const int *streams, const int *slots,
                                           const h264mi_tensor_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    return engine_export(e, n, streams, slots, desc, NULL, d_out, out_stride, stream);
}

// the same, resized (h264mi_tensor_resize_device_pitch)
extern "C" int h264mi_engine_export_tensor_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                   const h264mi_tensor_resize_desc *desc, void *d_out,
                                                   size_t out_stride, void *stream)
{
    return engine_export(e, n, streams, slots, desc ? &desc->t : NULL, desc, d_out, out_stride, stream);
}

// boxes over the frame slots (h264mi_tensor_rois_device_pitch; rois[r].pic
// indexes the n slots): one ordering of the two streams for the whole list
extern "C" int h264mi_engine_export_tensor_rois(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                const h264mi_tensor_resize_desc *desc, const h264mi_roi *rois,
                                                int nrois, void *d_out, size_t out_stride, void *stream)
{
    if (!e || n < 1 || !streams || !slots || !d_out) return -1;
    const int width = e->w * 16, height = e->h * 16;
    if (!rois_desc_ok(desc, rois, nrois, n, width, height)) return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->t.dtype), stream, [&] {
        std::vector<size_t> off((size_t)n);
        for (int k = 0; k < n; k++) off[k] = e->frame_bytes * ((size_t)streams[k] * e->nslots + slots[k]);
        return h264mi_tensor_rois_device_pitch(e->d_frames, off.data(), n, width, height, e->cpitch, desc, rois, nrois,
                                               d_out, out_stride, e->st);
    });
}

// the frame slots, or boxes over them, letterboxed (h264mi_tensor_fit_device_pitch,
// h264mi_tensor_rois_fit_device_pitch; rois == NULL: desc's window of every slot)
static int engine_export_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                             const h264mi_tensor_fit_desc *desc, const h264mi_roi *rois, int nrois, void *d_out,
                             size_t out_stride, void *stream)
{
    if (!e || n < 1 || !streams || !slots || !d_out) return -1;
    const int width = e->w * 16, height = e->h * 16;
    if (rois ? !rois_fit_desc_ok(desc, rois, nrois, n, width, height) : !fit_desc_ok(desc, width, height)) return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->r.t.dtype), stream, [&] {
        std::vector<size_t> off((size_t)n);
        for (int k = 0; k < n; k++) off[k] = e->frame_bytes * ((size_t)streams[k] * e->nslots + slots[k]);
        if (!rois)
            return h264mi_tensor_fit_device_pitch(e->d_frames, off.data(), n, width, height, e->cpitch, desc, d_out,
                                                  out_stride, e->st);
        return h264mi_tensor_rois_fit_device_pitch(e->d_frames, off.data(), n, width, height, e->cpitch, desc, rois,
                                                   nrois, d_out, out_stride, e->st);
    });
}

extern "C" int h264mi_engine_export_tensor_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                                               const h264mi_tensor_fit_desc *desc, void *d_out, size_t out_stride,
                                               void *stream)
{
    return engine_export_fit(e, n, streams, slots, desc, NULL, 0, d_out, out_stride, stream);
}

extern "C" int h264mi_engine_export_tensor_rois_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                    const h264mi_tensor_fit_desc *desc, const h264mi_roi *rois,
                                                    int nrois, void *d_out, size_t out_stride, void *stream)
{
    if (!rois) return -1;
    return engine_export_fit(e, n, streams, slots, desc, rois, nrois, d_out, out_stride, stream);
}

// the frame slots, or boxes over them, under a layout descriptor
// (h264mi_tensor_layout_device_pitch): one ordering of the two streams per call
// (dest, DESIGN §3.5p: judged before the streams are ordered, with the call's items)
extern "C" int h264mi_engine_export_tensor_dest(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois,
                                                int nrois, const h264mi_tensor_dest *dest, void *d_out,
                                                size_t out_stride, void *stream)
{
    if (!e || n < 1 || !streams || !slots || !d_out) return -1;
    const int width = e->w * 16, height = e->h * 16;
    if (!layout_desc_ok(desc, rois, nrois, n, width, height)) return -1;
    const h264mi_tensor_resize_desc &r = desc->f.r;
    const size_t es = export_elem_size(r.t.dtype);
    if (dest && !dest_ok(dest, es, H264MI_TENSOR_LAYOUT(r.t.mode) == H264MI_TENSOR_RGB ? 3 : 1,
                         layout_unresized(desc) ? r.t.ch : r.oh, layout_unresized(desc) ? r.t.cw : r.ow,
                         desc->layout == H264MI_LAYOUT_INTERLEAVED, rois ? nrois : n, out_stride))
        return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, es, stream, [&] {
        std::vector<size_t> off((size_t)n);
        for (int k = 0; k < n; k++) off[k] = e->frame_bytes * ((size_t)streams[k] * e->nslots + slots[k]);
        return h264mi_tensor_dest_device_pitch(e->d_frames, off.data(), n, width, height, e->cpitch, desc, rois, nrois,
                                               dest, d_out, out_stride, e->st);
    });
}

extern "C" int h264mi_engine_export_tensor_layout(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                  const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois,
                                                  int nrois, void *d_out, size_t out_stride, void *stream)
{
    return h264mi_engine_export_tensor_dest(e, n, streams, slots, desc, rois, nrois, NULL, d_out, out_stride, stream);
}

// warps over the frame slots (h264mi_tensor_warps_dest_device_pitch; warps[r].pic
// indexes the n slots): one ordering of the two streams for the whole list
extern "C" int h264mi_engine_export_tensor_warps_dest(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                      const h264mi_tensor_warp_desc *desc, const h264mi_warp *warps,
                                                      int nwarps, const h264mi_tensor_dest *dest, void *d_out,
                                                      size_t out_stride, void *stream)
{
    if (!e || n < 1 || !streams || !slots || !d_out) return -1;
    const int width = e->w * 16, height = e->h * 16;
    if (!warps_desc_ok(desc, warps, nwarps, n, width, height)) return -1;
    const size_t es = export_elem_size(desc->t.dtype);
    if (dest && !dest_ok(dest, es, H264MI_TENSOR_LAYOUT(desc->t.mode) == H264MI_TENSOR_RGB ? 3 : 1, desc->oh, desc->ow,
                         desc->layout == H264MI_LAYOUT_INTERLEAVED, nwarps, out_stride))
        return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, es, stream, [&] {
        std::vector<size_t> off((size_t)n);
        for (int k = 0; k < n; k++) off[k] = e->frame_bytes * ((size_t)streams[k] * e->nslots + slots[k]);
        return h264mi_tensor_warps_dest_device_pitch(e->d_frames, off.data(), n, width, height, e->cpitch, desc, warps,
                                                     nwarps, dest, d_out, out_stride, e->st);
    });
}

extern "C" int h264mi_engine_export_tensor_warps(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                 const h264mi_tensor_warp_desc *desc, const h264mi_warp *warps,
                                                 int nwarps, void *d_out, size_t out_stride, void *stream)
{
    return h264mi_engine_export_tensor_warps_dest(e, n, streams, slots, desc, warps, nwarps, NULL, d_out, out_stride, stream);
}

// Picture statistics (stats.hip, include/h264mi.h): item k -- desc's
// window of picture k, or box k of picture rois[k].pic -- as stats_item_words
// int64 words at d_out + k * out_stride, against the same window of reference
// picture k (rois: rois[k].pic) where d_ref names one.  Everything is checked
// first (common/export_desc.h: one bad box refuses the call); then, per
// EXPORT_MAX_PICS items, k_stats_init writes every word of their records and
// k_stats, behind it on the stream, adds the strips' partials -- the item
// offsets and windows travel in the kernel arguments.  rois is host memory, read
// here.  -1 (nothing launched) on a bad argument.
static_assert(H264MI_STATS_Y == STATS_Y && H264MI_STATS_YUV == STATS_YUV && H264MI_STATS_RGB == STATS_RGB &&
                  H264MI_STATS_WORDS == STATS_WORDS && H264MI_STATS_BINS == STATS_BINS &&
                  STATS_MAX_ITEMS == EXPORT_MAX_PICS,
              "include/h264mi.h and stats.hip name the same plane sets, record and items per launch");

extern "C" size_t h264mi_stats_item_words(const h264mi_stats_desc *desc) { return desc ? stats_item_words(desc) : 0; }

// a statistics descriptor, with its boxes (rois == NULL, then nrois == 0: its own window), an export accepts
static bool stats_desc_ok(const h264mi_stats_desc *d, const h264mi_roi *rois, int nrois, int npics, int width, int height)
{
    if (!d || (rois ? nrois < 1 : nrois != 0)) return false;
    if (rois) return stats_rois_ok(d, rois, nrois, npics, width, height);
    return stats_desc_fixed_ok(d) && stats_window_ok(d, width, height);
}

// d_out, out_stride: int64 words, and items that do not overlap
static bool stats_out_ok(const h264mi_stats_desc *d, int nitems, const void *d_out, size_t out_stride)
{
    return export_aligned(d_out, out_stride, 8) && (nitems < 2 || out_stride >= stats_item_words(d) * 8);
}

extern "C" int h264mi_stats_device_pitch(const void *d_in, const size_t *in_offsets, const void *d_ref,
                                         const size_t *ref_offsets, int npics, int width, int height, int cpitch,
                                         const h264mi_stats_desc *desc, const h264mi_roi *rois, int nrois, void *d_out,
                                         size_t out_stride, void *stream)
{
    if (!tensor_pics_ok(d_in, in_offsets, npics, width, height, cpitch, d_out) || !d_ref != !ref_offsets ||
        !stats_desc_ok(desc, rois, nrois, npics, width, height))
        return -1;
    const int nitems = rois ? nrois : npics;
    // (d_out is looked up too, as for the boxes of the pixel exports: a host address would fault every launch)
    if (!stats_out_ok(desc, nitems, d_out, out_stride) || h264mi_pointer_device(d_out) < 0) return -1;
    const bool hist = desc->flags & H264MI_STATS_HIST;
    stats_args a;
    a.in = (const uint8_t *)d_in;
    a.ref = (const uint8_t *)d_ref;
    a.out = (uint8_t *)d_out;
    a.width = width; a.height = height; a.cpitch = cpitch;
    a.col = tensor_colour_sets[desc->colour];       // (set 0 runs the kernel with the reference's literals)
    for (int k0 = 0; k0 < nitems; k0 += EXPORT_MAX_PICS) {
        const int n = nitems - k0 < EXPORT_MAX_PICS ? nitems - k0 : EXPORT_MAX_PICS;
        int strips = 1;
        for (int k = 0; k < EXPORT_MAX_PICS; k++) {
            const h264mi_roi w = {k0 + k, desc->x, desc->y, desc->cw, desc->ch};
            const h264mi_roi &b = rois ? rois[k0 + (k < n ? k : 0)] : w;
            const int pic = k < n ? b.pic : 0;
            a.in_off[k] = k < n ? in_offsets[pic] : 0;
            a.ref_off[k] = k < n && ref_offsets ? ref_offsets[pic] : 0;
            a.out_off[k] = k < n ? (size_t)(k0 + k) * out_stride : 0;
            a.win[k][0] = b.x; a.win[k][1] = b.y; a.win[k][2] = b.cw; a.win[k][3] = b.ch;
            const long long units = (long long)((b.cw + STATS_UNIT_COLS - 1) / STATS_UNIT_COLS) * (b.ch >> 1);
            const int s = (int)((units + STATS_STRIP_UNITS - 1) / STATS_STRIP_UNITS);
            if (k < n && s > strips) strips = s;
        }
        stats_launch(desc->planes, hist, d_ref != NULL, desc->colour != 0, strips, n, (hipStream_t)stream, a);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// statistics of the frame slots, or of boxes over them (rois[k].pic indexes the
// n slots), against the reference slots where named: one ordering of the two
// streams per call
extern "C" int h264mi_engine_export_stats(h264mi_engine *e, int n, const int *streams, const int *slots,
                                          const int *ref_streams, const int *ref_slots, const h264mi_stats_desc *desc,
                                          const h264mi_roi *rois, int nrois, void *d_out, size_t out_stride, void *stream)
{
    if (!e || n < 1 || !streams || !slots || !d_out || !ref_streams != !ref_slots) return -1;
    const int width = e->w * 16, height = e->h * 16;
    if (!stats_desc_ok(desc, rois, nrois, n, width, height) || !stats_out_ok(desc, rois ? nrois : n, d_out, out_stride))
        return -1;
    for (int k = 0; ref_streams && k < n; k++)
        if (ref_streams[k] < 0 || ref_streams[k] >= e->nstreams || ref_slots[k] < 0 || ref_slots[k] >= e->nslots) return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, 8, stream, [&] {
        std::vector<size_t> off((size_t)n), roff((size_t)n);
        for (int k = 0; k < n; k++) {
            off[k] = e->frame_bytes * ((size_t)streams[k] * e->nslots + slots[k]);
            if (ref_streams) roff[k] = e->frame_bytes * ((size_t)ref_streams[k] * e->nslots + ref_slots[k]);
        }
        return h264mi_stats_device_pitch(e->d_frames, off.data(), ref_streams ? e->d_frames : NULL,
                                         ref_streams ? roff.data() : NULL, n, width, height, e->cpitch, desc, rois, nrois,
                                         d_out, out_stride, e->st);
    });
}

// Motion vectors and MB side information as planar fields (mbinfo.hip): the
// window desc->(bx, by, bw, bh) of the 4x4-block grid of the npics record
// batches (w_mbs * h_mbs MbRec each) that start rec_offsets[k] bytes after
// d_recs, as contiguous (nch, bh, bw) elements of desc->dtype at d_out + k *
// out_stride; device pointers, asynchronous on `stream`; MBINFO_MAX_PICS
// pictures per launch.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_mbinfo_device(const void *d_recs, const size_t *rec_offsets, int npics, int w_mbs, int h_mbs,
                                    const h264mi_mbinfo_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    static_assert(H264MI_TENSOR_I16 == TENSOR_I16 && H264MI_MBINFO_MAX_CH == MBINFO_MAX_CH &&
                      H264MI_MBINFO_NCHANNELS == MBI_NCHANNELS && H264MI_MBINFO_MVX == MBI_MVX &&
                      H264MI_MBINFO_MVY == MBI_MVY && H264MI_MBINFO_REF_IDX == MBI_REF_IDX &&
                      H264MI_MBINFO_REF_SLOT == MBI_REF_SLOT && H264MI_MBINFO_MB_TYPE == MBI_MB_TYPE &&
                      H264MI_MBINFO_QP == MBI_QP && H264MI_MBINFO_INTRA_MODE == MBI_INTRA_MODE &&
                      H264MI_MBINFO_CODED == MBI_CODED && H264MI_MBINFO_SLICE == MBI_SLICE,
                  "include/h264mi.h and mbinfo.hip name the same channels and element types");
    if (!d_recs || !rec_offsets || !d_out || npics < 1 || w_mbs < 1 || h_mbs < 1 || w_mbs > 65535 || h_mbs > 65535 ||
        ((size_t)(uintptr_t)d_recs & 15) || !mbinfo_desc_ok(desc, w_mbs, h_mbs))
        return -1;
    for (int k = 0; k < npics; k++)
        if (rec_offsets[k] % sizeof(MbRec)) return -1;
    const size_t es = export_elem_size(desc->dtype);
    if (!export_aligned(d_out, out_stride, es)) return -1;
    const bool v16 = export_v16(d_out, out_stride, (size_t)desc->bw * es);
    mbinfo_args a;
    a.rec = (const uint8_t *)d_recs;
    a.w_mbs = w_mbs;
    a.bx = desc->bx; a.by = desc->by; a.bw = desc->bw; a.bh = desc->bh; a.nch = desc->nch;
    a.out_stride = out_stride;
    for (int c = 0; c < MBINFO_MAX_CH; c++) {
        a.ch[c] = c < desc->nch ? (uint8_t)desc->ch[c] : 0;
        a.scale[c] = c < desc->nch ? desc->scale[c] : 0.0f;
        a.bias[c] = c < desc->nch ? desc->bias[c] : 0.0f;
    }
    return export_launches(npics, rec_offsets, a.off, &a.out, d_out, out_stride,
                           [&](int, int n) { mbinfo_launch(desc->dtype, v16, n, (hipStream_t)stream, a); });
}

// Record retention: one batch per (stream, slot), 0xFF-filled ("no
// information") until a reconstruction into the slot copies its records there
// (keep_batch).  Off waits for the engine's stream (exports run on it) and frees.
// (One batch more than the slots: it is never copied into, and
// h264mi_engine_export_residual reads it for a slot whose coefficients it does
// not hold.)  keep_hold is the switch itself; the records are held while the
// caller's switch or coefficient retention is on.
static int keep_hold(h264mi_engine *e, int on)
{
    if ((on != 0) == (e->exp.d_keep != NULL)) return 0;
    HIPCHECK(hipSetDevice(e->dev));
    const size_t bytes = sizeof(MbRec) * e->nmbs * ((size_t)e->nslots * e->nstreams + 1);
    if (on) {
        HIPCHECK(hipMalloc(&e->exp.d_keep, bytes));
        if (hipMemsetAsync(e->exp.d_keep, 0xFF, bytes, e->st) != hipSuccess) {
            (void)hipFree(e->exp.d_keep);
            e->exp.d_keep = NULL;
            return -1;
        }
        return 0;
    }
    HIPCHECK(hipStreamSynchronize(e->st));
    (void)hipFree(e->exp.d_keep);
    e->exp.d_keep = NULL;
    return 0;
}

extern "C" int h264mi_engine_keep_records(h264mi_engine *e, int on)
{
    if (!e) return -1;
    e->exp.keep_rec = on != 0;
    return keep_hold(e, e->exp.keep_rec || e->exp.d_keepc);
}

// Coefficient retention: one worst-case batch per (stream, slot), filled by
// keep_coef_batch; it holds the records as well while it is on.  A slot's
// blocks count only with the records of the same reconstruction, so switching
// on starts with no slot valid.  Off waits for the engine's stream and frees.
extern "C" int h264mi_engine_keep_coefs(h264mi_engine *e, int on)
{
    if (!e) return -1;
    if ((on != 0) == (e->exp.d_keepc != NULL)) return 0;
    HIPCHECK(hipSetDevice(e->dev));
    if (on) {
        const size_t nb = (size_t)e->nslots * e->nstreams;
        if (keep_hold(e, 1)) return -1;
        e->exp.keepc_ok = (uint8_t *)calloc(nb, 1);
        if (!e->exp.keepc_ok || hipMalloc(&e->exp.d_keepc, nb * keepc_cap(e) * 32) != hipSuccess) {
            free(e->exp.keepc_ok);
            e->exp.keepc_ok = NULL;
            e->exp.d_keepc = NULL;
            (void)keep_hold(e, e->exp.keep_rec);
            return -1;
        }
        return 0;
    }
    HIPCHECK(hipStreamSynchronize(e->st));
    (void)hipFree(e->exp.d_keepc);
    free(e->exp.keepc_ok);
    e->exp.d_keepc = NULL;
    e->exp.keepc_ok = NULL;
    return keep_hold(e, e->exp.keep_rec);
}

extern "C" int h264mi_engine_forget_records(h264mi_engine *e, int stream, int slot)
{
    if (!e || (!e->exp.d_keep && !e->exp.d_acc) || stream < 0 || stream >= e->nstreams || slot < 0 || slot >= e->nslots)
        return -1;
    HIPCHECK(hipSetDevice(e->dev));
    if (e->exp.keepc_ok) e->exp.keepc_ok[(size_t)stream * e->nslots + slot] = 0;
    if (e->exp.d_keep)
        HIPCHECK(hipMemsetAsync(e->exp.d_keep + ((size_t)stream * e->nslots + slot) * e->nmbs, 0xFF, sizeof(MbRec) * e->nmbs, e->st));
    if (e->exp.d_acc) {
        // the slot's map says nothing about its picture: none as a reference, (x, y, 0) when exported
        e->exp.acc_ser[(size_t)stream * e->nslots + slot] = 0;
        if (e->exp.akey_slot && e->exp.akey_slot[stream] == slot) e->exp.akey_slot[stream] = -1;    // (its entry stays: the GOP's pictures export against it)
        return accmv_clear(e, (size_t)stream * e->nslots + slot, 1);
    }
    return 0;
}

// The kept batches of the slots (streams[k], slots[k]) as fields in the
// caller's memory, ordered between the caller's stream and ours by export_ordered
extern "C" int h264mi_engine_export_mbinfo(h264mi_engine *e, int n, const int *streams, const int *slots,
                                           const h264mi_mbinfo_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    if (!e || !e->exp.d_keep || n < 1 || !streams || !slots || !d_out || !mbinfo_desc_ok(desc, e->w, e->h)) return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->dtype), stream, [&] {
        std::vector<size_t> off((size_t)n);
        for (int k = 0; k < n; k++) off[k] = sizeof(MbRec) * e->nmbs * ((size_t)streams[k] * e->nslots + slots[k]);
        return h264mi_mbinfo_device(e->exp.d_keep, off.data(), n, e->w, e->h, desc, d_out, out_stride, e->st);
    });
}

// The decoded residual as planar tensors (residual.hip): the window desc->(x,
// y, cw, ch), in luma samples of the MB-aligned picture, of the npics pictures
// whose record batches (w_mbs * h_mbs MbRec each) start rec_offsets[k] bytes
// after d_recs and whose coefficient blocks start coef_bases[k] blocks after
// d_coef, a pool of coef_blocks blocks; picture k's planes, contiguous, at
// d_out + k * out_stride; device pointers, asynchronous on `stream`;
// RESID_MAX_PICS pictures per launch.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_residual_device(const void *d_recs, const size_t *rec_offsets, const void *d_coef,
                                      const uint32_t *coef_bases, size_t coef_blocks, int npics, int w_mbs, int h_mbs,
                                      const h264mi_residual_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    static_assert(H264MI_RESID_Y == RESID_Y && H264MI_RESID_UV == RESID_UV && H264MI_RESID_YUV == RESID_YUV,
                  "include/h264mi.h and residual.hip name the same planes");
    if (!d_recs || !rec_offsets || !d_coef || !coef_bases || !d_out || npics < 1 || w_mbs < 1 || h_mbs < 1 ||
        w_mbs > 65535 || h_mbs > 65535 || (((size_t)(uintptr_t)d_recs | (size_t)(uintptr_t)d_coef) & 15) ||
        !residual_desc_ok(desc, w_mbs, h_mbs))
        return -1;
    for (int k = 0; k < npics; k++)
        if (rec_offsets[k] % sizeof(MbRec)) return -1;
    const size_t es = export_elem_size(desc->dtype);
    if (!export_aligned(d_out, out_stride, es)) return -1;
    const bool v16 = export_v16(d_out, out_stride, (size_t)(desc->planes == H264MI_RESID_UV ? desc->cw / 2 : desc->cw) * es);
    residual_args a;
    a.rec = (const uint8_t *)d_recs;
    a.coef = (const int16_t *)d_coef;
    a.coef_blocks = coef_blocks;
    a.w_mbs = w_mbs;
    a.x = desc->x; a.y = desc->y; a.cw = desc->cw; a.ch = desc->ch; a.planes = desc->planes;
    a.out_stride = out_stride;
    for (int c = 0; c < 3; c++) { a.scale[c] = desc->scale[c]; a.bias[c] = desc->bias[c]; }
    return export_launches(npics, rec_offsets, a.off, &a.out, d_out, out_stride, [&](int k0, int n) {
        for (int k = 0; k < RESID_MAX_PICS; k++) a.cbase[k] = k < n ? coef_bases[k0 + k] : 0;
        residual_launch(desc->dtype, v16, n, (hipStream_t)stream, a);
    });
}

// The kept records and coefficients of the slots (streams[k], slots[k]) as
// residual tensors in the caller's memory, ordered like
// h264mi_engine_export_mbinfo.  A slot whose coefficients are not held (nothing
// decoded into it since retention went on, forgotten, or more blocks than a
// batch holds) reads the spare 0xFF record batch: zeros.
extern "C" int h264mi_engine_export_residual(h264mi_engine *e, int n, const int *streams, const int *slots,
                                             const h264mi_residual_desc *desc, void *d_out, size_t out_stride,
                                             void *stream)
{
    if (!e || !e->exp.d_keepc || !e->exp.d_keep || n < 1 || !streams || !slots || !d_out || !residual_desc_ok(desc, e->w, e->h))
        return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->dtype), stream, [&] {
        const size_t nb = (size_t)e->nslots * e->nstreams;
        std::vector<size_t> off((size_t)n);
        std::vector<uint32_t> cbase((size_t)n);
        for (int k = 0; k < n; k++) {
            const size_t b = (size_t)streams[k] * e->nslots + slots[k];
            off[k] = sizeof(MbRec) * e->nmbs * (e->exp.keepc_ok[b] ? b : nb);
            cbase[k] = (uint32_t)(b * keepc_cap(e));
        }
        return h264mi_residual_device(e->exp.d_keep, off.data(), e->exp.d_keepc, cbase.data(), nb * keepc_cap(e), n, e->w, e->h,
                                      desc, d_out, out_stride, e->st);
    });
}

// an export descriptor h264mi_accmv_device accepts on a w_mbs x h_mbs picture
static bool accmv_desc_ok(const h264mi_accmv_desc *d, int w_mbs, int h_mbs)
{
    return d && accmv_desc_fixed_ok(d) && accmv_window_ok(d, w_mbs, h_mbs);
}

// One step of the accumulated motion (accmv.hip k_accmv_step): the origin map
// of the picture whose records start at d_recs, from the maps d_ref_maps[s] of
// the slots it references (NULL: none) or, with key != 0, the identity.  Device
// pointers, asynchronous on `stream`.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_accmv_step_device(const void *d_recs, int w_mbs, int h_mbs, const void *const *d_ref_maps,
                                        int nslots, int key, void *d_map_out, void *stream)
{
    static_assert(H264MI_ACCMV_MAX_SLOTS == ACCMV_MAX_SLOTS && H264MI_ACCMV_MAX_CH == ACCMV_MAX_CH &&
                      H264MI_ACCMV_NCHANNELS == ACC_NCHANNELS && H264MI_ACCMV_ADX == ACC_ADX &&
                      H264MI_ACCMV_ADY == ACC_ADY && H264MI_ACCMV_JX == ACC_JX && H264MI_ACCMV_JY == ACC_JY &&
                      H264MI_ACCMV_ANCHORED == ACC_ANCHORED && ACCMV_MAX_PICS == EXPORT_MAX_PICS,
                  "include/h264mi.h and accmv.hip name the same channels and bounds");
    if (!d_recs || !d_map_out || !accmv_size_ok(w_mbs, h_mbs) || nslots < 0 || nslots > ACCMV_MAX_SLOTS ||
        (nslots && !d_ref_maps) || (((size_t)(uintptr_t)d_recs | (size_t)(uintptr_t)d_map_out) & 15))
        return -1;
    for (int s = 0; s < nslots; s++)
        if (d_ref_maps[s] == d_map_out || ((size_t)(uintptr_t)d_ref_maps[s] & 3)) return -1;
    accmv_step_args a;
    memset(&a, 0, sizeof(a));
    a.rec = (const uint8_t *)d_recs;
    a.w_mbs = w_mbs; a.W = 16 * w_mbs; a.H = 16 * h_mbs; a.nslots = nslots;
    a.out[0] = (uint32_t *)d_map_out;
    for (int s = 0; s < nslots; s++) a.ref[0][s] = (const uint32_t *)d_ref_maps[s];
    a.mode[0] = key ? ACCMV_KEY : ACCMV_STEP;
    accmv_step_launch(1, (hipStream_t)stream, a);
    HIPCHECK(hipGetLastError());
    return 0;
}

// a resized export's descriptor h264mi_accmv_resize_device accepts on a w_mbs x h_mbs picture
static bool accmv_resize_desc_ok(const h264mi_accmv_resize_desc *d, int w_mbs, int h_mbs)
{
    return d && accmv_resize_fixed_ok(d) && accmv_resize_window_ok(d, w_mbs, h_mbs);
}

// Both accumulated-motion exports (r != NULL: resized, desc = &r->f): one check
// and one fill of what their kernels share, accmv_args
static int accmv_device(const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                        const h264mi_accmv_desc *desc, const h264mi_accmv_resize_desc *r, void *d_out,
                        size_t out_stride, void *stream)
{
    if (!d_maps || !map_offsets || !d_out || npics < 1 || ((size_t)(uintptr_t)d_maps & 3) ||
        (r ? !accmv_resize_desc_ok(r, w_mbs, h_mbs) : !accmv_desc_ok(desc, w_mbs, h_mbs)))
        return -1;
    for (int k = 0; k < npics; k++)
        if (map_offsets[k] & 3) return -1;
    const size_t es = export_elem_size(desc->dtype);
    if (!export_aligned(d_out, out_stride, es)) return -1;
    const bool v16 = export_v16(d_out, out_stride, (size_t)desc->cw * es);
    fresize_args<fresize_accmv> ra;
    accmv_args &a = ra.f;
    a.maps = (const uint8_t *)d_maps;
    a.W = 16 * w_mbs;
    a.x = desc->x; a.y = desc->y; a.cw = desc->cw; a.ch = desc->ch; a.nch = desc->nch;
    a.out_stride = out_stride;
    for (int c = 0; c < ACCMV_MAX_CH; c++) {
        a.id[c] = c < desc->nch ? (uint8_t)desc->id[c] : 0;
        a.scale[c] = c < desc->nch ? desc->scale[c] : 0.0f;
        a.bias[c] = c < desc->nch ? desc->bias[c] : 0.0f;
    }
    ra.ow = r ? r->ow : 0; ra.oh = r ? r->oh : 0;
    return export_launches(npics, map_offsets, a.off, &a.out, d_out, out_stride, [&](int, int n) {
        if (r) fresize_launch(desc->dtype, n, (hipStream_t)stream, ra);
        else accmv_launch(desc->dtype, v16, n, (hipStream_t)stream, a);
    });
}

// Origin maps as planar channels (accmv.hip k_accmv): the window desc->(x, y,
// cw, ch) of the npics maps (16 * w_mbs words a row) that start map_offsets[k]
// bytes after d_maps, as contiguous (nch, ch, cw) elements of desc->dtype at
// d_out + k * out_stride; device pointers, asynchronous on `stream`;
// ACCMV_MAX_PICS pictures per launch.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_accmv_device(const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                                   const h264mi_accmv_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    return accmv_device(d_maps, map_offsets, npics, w_mbs, h_mbs, desc, NULL, d_out, out_stride, stream);
}

// The same fields resized (field_resize.hip): the window's integer field
// filtered to desc->oh x desc->ow samples per channel, picture k's (nch, oh, ow)
// elements at d_out + k * out_stride.  The window is at most 16384 a side and
// 32 times the output on each axis.  Stateless: the tap tables are made in the
// kernel.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_accmv_resize_device(const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                                          const h264mi_accmv_resize_desc *desc, void *d_out, size_t out_stride,
                                          void *stream)
{
    return accmv_device(d_maps, map_offsets, npics, w_mbs, h_mbs, desc ? &desc->f : NULL, desc, d_out, out_stride, stream);
}

// the maps of slots [first, first + n) of the engine's pool as (x, y, 0), on its stream
static int accmv_clear(h264mi_engine *e, size_t first, size_t n)
{
    accmv_step_args a;
    memset(&a, 0, sizeof(a));
    a.w_mbs = e->w; a.W = 16 * e->w; a.H = 16 * e->h;
    for (size_t k0 = 0; k0 < n; k0 += ACCMV_STEP_PICS) {
        const int m = n - k0 < ACCMV_STEP_PICS ? (int)(n - k0) : ACCMV_STEP_PICS;
        for (int k = 0; k < ACCMV_STEP_PICS; k++) {
            a.out[k] = e->exp.d_acc + (first + k0 + (k < m ? k : 0)) * acc_words(e);
            a.mode[k] = ACCMV_CLEAR;
        }
        accmv_step_launch(m, e->st, a);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// Origin-map retention: one map per (stream, slot), (x, y, 0) until a
// reconstruction into the slot steps into it (accmv_batch); every serial starts
// at 0, so switching on starts from nothing.  Off waits for the engine's stream
// (exports run on it) and frees.
extern "C" int h264mi_engine_keep_accmv(h264mi_engine *e, int on)
{
    if (!e) return -1;
    if ((on != 0) == (e->exp.d_acc != NULL)) return 0;
    HIPCHECK(hipSetDevice(e->dev));
    if (on) {
        if (!accmv_size_ok(e->w, e->h) || e->nslots > ACCMV_MAX_SLOTS) return -1;
        const size_t nb = (size_t)e->nslots * e->nstreams;
        e->exp.acc_key = (unsigned long long *)calloc((size_t)e->nstreams, sizeof(unsigned long long));
        e->exp.acc_ser = (unsigned long long *)calloc(nb, sizeof(unsigned long long));
        if (!e->exp.acc_key || !e->exp.acc_ser || hipMalloc(&e->exp.d_acc, nb * acc_words(e) * 4) != hipSuccess ||
            accmv_clear(e, 0, nb)) {
            (void)hipStreamSynchronize(e->st);
            (void)hipFree(e->exp.d_acc);
            free(e->exp.acc_key); free(e->exp.acc_ser);
            e->exp.d_acc = NULL; e->exp.acc_key = e->exp.acc_ser = NULL;
            return -1;
        }
        return 0;
    }
    if (h264mi_engine_keep_accres(e, 0)) return -1;     // the keys go with the maps they are read through
    HIPCHECK(hipStreamSynchronize(e->st));
    (void)hipFree(e->exp.d_acc);
    free(e->exp.acc_key); free(e->exp.acc_ser);
    e->exp.d_acc = NULL; e->exp.acc_key = e->exp.acc_ser = NULL;
    return 0;
}

// The kept maps of the slots (streams[k], slots[k]) as tensors in the caller's
// memory, ordered between the caller's stream and ours by export_ordered
static int engine_export_accmv(h264mi_engine *e, int n, const int *streams, const int *slots,
                               const h264mi_accmv_desc *desc, const h264mi_accmv_resize_desc *rdesc, void *d_out,
                               size_t out_stride, void *stream)
{
    if (!e || !e->exp.d_acc || n < 1 || !streams || !slots || !d_out ||
        (rdesc ? !accmv_resize_desc_ok(rdesc, e->w, e->h) : !accmv_desc_ok(desc, e->w, e->h)))
        return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->dtype), stream, [&] {
        std::vector<size_t> off((size_t)n);
        for (int k = 0; k < n; k++) off[k] = acc_words(e) * 4 * ((size_t)streams[k] * e->nslots + slots[k]);
        return accmv_device(e->exp.d_acc, off.data(), n, e->w, e->h, desc, rdesc, d_out, out_stride, e->st);
    });
}

extern "C" int h264mi_engine_export_accmv(h264mi_engine *e, int n, const int *streams, const int *slots,
                                          const h264mi_accmv_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    return engine_export_accmv(e, n, streams, slots, desc, NULL, d_out, out_stride, stream);
}

// the same, resized (h264mi_accmv_resize_device)
extern "C" int h264mi_engine_export_accmv_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                  const h264mi_accmv_resize_desc *desc, void *d_out, size_t out_stride,
                                                  void *stream)
{
    return engine_export_accmv(e, n, streams, slots, desc ? &desc->f : NULL, desc, d_out, out_stride, stream);
}

// an export descriptor h264mi_accres_device accepts on a w_mbs x h_mbs picture
static bool accres_desc_ok(const h264mi_accres_desc *d, int w_mbs, int h_mbs)
{
    return d && accres_desc_fixed_ok(d) && accres_window_ok(d, w_mbs, h_mbs);
}

// a resized export's descriptor h264mi_accres_resize_device accepts on a w_mbs x h_mbs picture
static bool accres_resize_desc_ok(const h264mi_accres_resize_desc *d, int w_mbs, int h_mbs)
{
    return d && accres_resize_fixed_ok(d) && accres_resize_window_ok(d, w_mbs, h_mbs);
}

// Both accumulated-residual exports (r != NULL: resized, desc = &r->f): one
// check and one fill of what their kernels share, accres_args
static int accres_device(const void *d_cur, const size_t *cur_offsets, const void *d_key, const size_t *key_offsets,
                         const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                         const h264mi_accres_desc *desc, const h264mi_accres_resize_desc *r, void *d_out,
                         size_t out_stride, void *stream)
{
    static_assert(H264MI_ACCRES_Y == ACCRES_Y && H264MI_ACCRES_UV == ACCRES_UV && H264MI_ACCRES_YUV == ACCRES_YUV &&
                      H264MI_ACCRES_RGB == ACCRES_RGB && ACCRES_MAX_PICS == EXPORT_MAX_PICS &&
                      H264MI_TENSOR_COLOUR_BT709_FULL == TENSOR_COLOUR_SETS - 1,
                  "include/h264mi.h and accres.hip name the same planes, bounds and colour sets");
    if (!d_cur || !cur_offsets || !key_offsets || !d_maps || !map_offsets || !d_out || npics < 1 ||
        (((size_t)(uintptr_t)d_cur | (size_t)(uintptr_t)d_key | (size_t)(uintptr_t)d_maps) & 3) ||
        (r ? !accres_resize_desc_ok(r, w_mbs, h_mbs) : !accres_desc_ok(desc, w_mbs, h_mbs)))
        return -1;
    for (int k = 0; k < npics; k++) {
        if ((map_offsets[k] | cur_offsets[k]) & 3) return -1;
        if (key_offsets[k] != (size_t)-1 && (!d_key || (key_offsets[k] & 3))) return -1;
    }
    const size_t es = export_elem_size(desc->dtype);
    if (!export_aligned(d_out, out_stride, es)) return -1;
    const int ow = desc->planes == H264MI_ACCRES_UV ? desc->cw / 2 : desc->cw;
    const bool v16 = export_v16(d_out, out_stride, (size_t)ow * es);
    fresize_args<fresize_accres> ra;
    accres_args &a = ra.f;
    a.cur = (const uint8_t *)d_cur; a.key = (const uint8_t *)d_key; a.maps = (const uint8_t *)d_maps;
    a.W = 16 * w_mbs; a.H = 16 * h_mbs; a.cpitch = H264MI_CPITCH(w_mbs);
    a.x = desc->x; a.y = desc->y; a.cw = desc->cw; a.ch = desc->ch;
    a.planes = desc->planes; a.zero = desc->unanchored == H264MI_ACCRES_ZERO;
    a.out_stride = out_stride;
    a.col = tensor_colour_sets[desc->colour];
    for (int c = 0; c < 3; c++) { a.scale[c] = desc->scale[c]; a.bias[c] = desc->bias[c]; }
    ra.ow = r ? r->ow : 0; ra.oh = r ? r->oh : 0;
    return export_launches(npics, map_offsets, a.map_off, &a.out, d_out, out_stride, [&](int k0, int n) {
        for (int k = 0; k < ACCRES_MAX_PICS; k++) {
            a.cur_off[k] = k < n ? cur_offsets[k0 + k] : 0;
            a.key_off[k] = k < n && key_offsets[k0 + k] != (size_t)-1 ? key_offsets[k0 + k] : ACCRES_NO_KEY;
        }
        if (r) fresize_launch(desc->dtype, n, (hipStream_t)stream, ra);
        else accres_launch(desc->dtype, v16, n, (hipStream_t)stream, a);
    });
}

// The accumulated residual (accres.hip k_accres): the window desc->(x, y, cw,
// ch) of npics pictures -- frame, key frame or none ((size_t)-1), origin map,
// each at its offset -- as contiguous (planes, ch, cw) elements of desc->dtype
// at d_out + k * out_stride; device pointers, asynchronous on `stream`;
// ACCRES_MAX_PICS pictures per launch.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_accres_device(const void *d_cur, const size_t *cur_offsets, const void *d_key,
                                    const size_t *key_offsets, const void *d_maps, const size_t *map_offsets, int npics,
                                    int w_mbs, int h_mbs, const h264mi_accres_desc *desc, void *d_out, size_t out_stride,
                                    void *stream)
{
    return accres_device(d_cur, cur_offsets, d_key, key_offsets, d_maps, map_offsets, npics, w_mbs, h_mbs, desc, NULL,
                         d_out, out_stride, stream);
}

// The same fields resized (field_resize.hip): the window's integer field (UV:
// its half-resolution grid) filtered to desc->oh x desc->ow samples per plane,
// picture k's (planes, oh, ow) elements at d_out + k * out_stride; the bounds of
// h264mi_accmv_resize_device on the grid.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_accres_resize_device(const void *d_cur, const size_t *cur_offsets, const void *d_key,
                                           const size_t *key_offsets, const void *d_maps, const size_t *map_offsets,
                                           int npics, int w_mbs, int h_mbs, const h264mi_accres_resize_desc *desc,
                                           void *d_out, size_t out_stride, void *stream)
{
    return accres_device(d_cur, cur_offsets, d_key, key_offsets, d_maps, map_offsets, npics, w_mbs, h_mbs,
                         desc ? &desc->f : NULL, desc, d_out, out_stride, stream);
}

static void accres_free(h264mi_engine *e)
{
    (void)hipFree(e->exp.d_akey);
    free(e->exp.akey_tag); free(e->exp.akey_slot);
    e->exp.d_akey = NULL; e->exp.akey_tag = NULL; e->exp.akey_slot = NULL;
    e->exp.akey_n = 0;
}

// Key-picture retention: nkeys frames per stream, none tagged, so switching on
// starts from nothing (pictures decoded before have no key).  Off, and a change
// of nkeys, wait for the engine's stream (copies and exports run on it) and free.
extern "C" int h264mi_engine_keep_accres(h264mi_engine *e, int nkeys)
{
    if (!e || nkeys < 0 || nkeys > H264MI_ACCRES_MAX_KEYS) return -1;
    if (nkeys == e->exp.akey_n) return 0;
    if (nkeys && !e->exp.d_acc) return -1;          // a key is read through an origin map
    HIPCHECK(hipSetDevice(e->dev));
    if (e->exp.akey_n) {
        HIPCHECK(hipStreamSynchronize(e->st));
        accres_free(e);
    }
    if (!nkeys) return 0;
    const size_t ne = (size_t)e->nstreams * nkeys;
    e->exp.akey_tag = (unsigned long long *)calloc(ne, sizeof(unsigned long long));
    e->exp.akey_slot = (int *)malloc(sizeof(int) * (size_t)e->nstreams);
    if (!e->exp.akey_tag || !e->exp.akey_slot || hipMalloc(&e->exp.d_akey, ne * e->frame_bytes) != hipSuccess) {
        e->exp.d_akey = NULL;
        accres_free(e);
        return -1;
    }
    for (int s = 0; s < e->nstreams; s++) e->exp.akey_slot[s] = -1;
    e->exp.akey_n = nkeys;
    return 0;
}

// the entry that holds the key of the slot's picture, or -1: the slot's map
// carries serial t, and entry t % akey_n holds that key iff it is tagged t
static long accres_entry(const h264mi_engine *e, int stream, int slot)
{
    const unsigned long long t = e->exp.acc_ser[(size_t)stream * e->nslots + slot];
    const size_t entry = (size_t)stream * e->exp.akey_n + (size_t)(t % (unsigned)e->exp.akey_n);
    return t && e->exp.akey_tag[entry] == t ? (long)entry : -1;
}

extern "C" int h264mi_engine_accres_held(h264mi_engine *e, int stream, int slot)
{
    if (!e || !e->exp.d_akey || stream < 0 || stream >= e->nstreams || slot < 0 || slot >= e->nslots) return -1;
    return accres_entry(e, stream, slot) >= 0;
}

// The accumulated residual of the slots (streams[k], slots[k]) against the keys
// held for them, as tensors in the caller's memory, ordered between the
// caller's stream and ours by export_ordered
static int engine_export_accres(h264mi_engine *e, int n, const int *streams, const int *slots,
                                const h264mi_accres_desc *desc, const h264mi_accres_resize_desc *rdesc, void *d_out,
                                size_t out_stride, void *stream)
{
    if (!e || !e->exp.d_akey || n < 1 || !streams || !slots || !d_out ||
        (rdesc ? !accres_resize_desc_ok(rdesc, e->w, e->h) : !accres_desc_ok(desc, e->w, e->h)))
        return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->dtype), stream, [&] {
        std::vector<size_t> cur((size_t)n), key((size_t)n), map((size_t)n);
        for (int k = 0; k < n; k++) {
            const size_t b = (size_t)streams[k] * e->nslots + slots[k];
            const long entry = accres_entry(e, streams[k], slots[k]);
            cur[k] = e->frame_bytes * b;
            key[k] = entry < 0 ? (size_t)-1 : e->frame_bytes * (size_t)entry;
            map[k] = acc_words(e) * 4 * b;
        }
        return accres_device(e->d_frames, cur.data(), e->exp.d_akey, key.data(), e->exp.d_acc, map.data(), n, e->w, e->h, desc,
                             rdesc, d_out, out_stride, e->st);
    });
}

extern "C" int h264mi_engine_export_accres(h264mi_engine *e, int n, const int *streams, const int *slots,
                                           const h264mi_accres_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    return engine_export_accres(e, n, streams, slots, desc, NULL, d_out, out_stride, stream);
}

// the same, resized (h264mi_accres_resize_device), under the same held-key rule
extern "C" int h264mi_engine_export_accres_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                   const h264mi_accres_resize_desc *desc, void *d_out,
                                                   size_t out_stride, void *stream)
{
    return engine_export_accres(e, n, streams, slots, desc ? &desc->f : NULL, desc, d_out, out_stride, stream);
}
