/* Broadway decoder API (H264SwDec*) and wasm/JS glue (broadway*) on top of
 * the host decoder + HIP reconstruction backend.
 *
 * H264SwDec*: same structures, return codes and call protocol as the
 * reference Decoder/src/H264SwDecApi.c (Init :124-180, GetInfo :204-257,
 * Release :259-290, Decode :338-473, GetAPIVersion :487-500,
 * NextPicture :524-569).  broadway*: same behaviour as Decoder/src/Decoder.c
 * (playStream loop :44-53, broadwayDecode :100-162 incl. dropping the rest of
 * the buffer after a picture, :122-134), with the emscripten imports
 * broadwayOnHeadersDecoded / broadwayOnPictureDecoded delivered through
 * callbacks registered by broadwaySetCallbacks.
 *
 * The product path has no CPU reconstruction: if the HIP backend cannot be
 * created the API fails (H264SWDEC_INITFAIL / MEMFAIL) instead of falling
 * back. */
#include "../../../include/h264mi.h"
#include "../common/export_desc.h"
#include "decoder.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

H264Backend h264mi_hip_backend_create(int device);

/* ---- application hooks (reference inc/H264SwDecApi.h:160-173) ----------
 * The library allocates and frees its instances through H264SwDecMalloc /
 * H264SwDecFree and fills them with H264SwDecMemset, as H264SwDecApi.c:147,
 * :301 does; H264SwDecTrace receives the API trace strings when built with
 * -DH264DEC_TRACE (H264SwDecApi.c:66-72).  These are the reference's default
 * definitions (H264SwDecApi.c:78-96): an application that defines its own
 * (DecTestBench.c:678-760, TestBenchMultipleInstance.c:396-446) overrides them
 * by ordinary ELF symbol interposition -- the library calls them through its
 * PLT. */
void H264SwDecTrace(char *string) { (void)string; }
void *H264SwDecMalloc(u32 size) { return malloc(size); }
void H264SwDecFree(void *ptr) { free(ptr); }
void H264SwDecMemcpy(void *dest, void *src, u32 count) { memcpy(dest, src, count); }
void H264SwDecMemset(void *ptr, i32 value, u32 count) { memset(ptr, value, count); }

#ifdef H264DEC_TRACE
#define DEC_API_TRC(str) H264SwDecTrace((char *)(str))
#else
#define DEC_API_TRC(str) ((void)0)
#endif

enum { ST_UNINIT = 0, ST_INIT = 1, ST_NEW_HEADERS = 2 };

typedef struct DecContainer {
    H264Dec dec;
    int     stat;
    u32     pic_number;
} DecContainer;

static int backend_device(void)
{
    const char *s = getenv("H264MI_DEVICE");
    return s ? atoi(s) : 0;
}

H264SwDecRet H264SwDecInit(H264SwDecInst *decInst, u32 noOutputReordering)
{
    DEC_API_TRC("H264SwDecInit#");
    if (decInst == NULL) {
        DEC_API_TRC("H264SwDecInit# ERROR: decInst == NULL");
        return H264SWDEC_PARAM_ERR;
    }
    *decInst = NULL;
    DecContainer *c = (DecContainer *)H264SwDecMalloc((u32)sizeof(DecContainer));
    if (!c) {
        DEC_API_TRC("H264SwDecInit# ERROR: Memory allocation failed");
        return H264SWDEC_MEMFAIL;
    }
    H264SwDecMemset(c, 0, (u32)sizeof(DecContainer));
    H264Backend be = h264mi_hip_backend_create(backend_device());
    if (!be.ctx) { H264SwDecFree(c); return H264SWDEC_MEMFAIL; }
    if (h264dec_init(&c->dec, (int)noOutputReordering, be)) {
        be.destroy(be.ctx);
        H264SwDecFree(c);
        return H264SWDEC_INITFAIL;
    }
    c->stat = ST_INIT;
    *decInst = c;
    DEC_API_TRC("H264SwDecInit# OK");
    return H264SWDEC_OK;
}

H264SwDecRet H264SwDecGetInfo(H264SwDecInst decInst, H264SwDecInfo *pDecInfo)
{
    DEC_API_TRC("H264SwDecGetInfo#");
    if (decInst == NULL || pDecInfo == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    const Sps *s = h264dec_active_sps(&c->dec);
    if (!s || c->dec.active_pps < 0 || c->dec.active_pps >= MAX_PPS) return H264SWDEC_HDRS_NOT_RDY;
    memset(pDecInfo, 0, sizeof(*pDecInfo));
    pDecInfo->picWidth = (u32)s->w_mbs << 4;
    pDecInfo->picHeight = (u32)s->h_mbs << 4;
    pDecInfo->videoRange = (s->vui_present && s->video_full_range) ? 1 : 0;
    pDecInfo->matrixCoefficients = (s->vui_present && s->colour_desc_present) ? (u32)s->matrix_coeffs : 2;
    if (s->crop) {
        const export_window w = sps_crop_window(s);
        pDecInfo->croppingFlag = 1;
        pDecInfo->cropParams.cropLeftOffset = (u32)w.x;
        pDecInfo->cropParams.cropOutWidth = (u32)w.cw;
        pDecInfo->cropParams.cropTopOffset = (u32)w.y;
        pDecInfo->cropParams.cropOutHeight = (u32)w.ch;
    }
    u32 w = 1, h = 1;
    if (s->vui_present && s->aspect_present) {
        static const u8 sar[17][2] = {{0, 0}, {1, 1}, {12, 11}, {10, 11}, {16, 11}, {40, 33}, {24, 11},
                                      {20, 11}, {32, 11}, {80, 33}, {18, 11}, {15, 11}, {64, 33},
                                      {160, 99}, {0, 0}, {0, 0}, {0, 0}};
        if (s->aspect_idc == 255) {
            w = (u32)s->sar_w; h = (u32)s->sar_h;
            if (!w || !h) w = h = 0;
        } else if (s->aspect_idc < 14) {
            w = sar[s->aspect_idc][0]; h = sar[s->aspect_idc][1];
        } else {
            w = h = 0;
        }
    }
    pDecInfo->parWidth = w;
    pDecInfo->parHeight = h;
    pDecInfo->profile = (u32)s->profile_idc;
    return H264SWDEC_OK;
}

void H264SwDecRelease(H264SwDecInst decInst)
{
    if (!decInst) return;
    DEC_API_TRC("H264SwDecRelease#");
    DecContainer *c = (DecContainer *)decInst;
    h264dec_release(&c->dec);
    H264SwDecFree(c);
}

H264SwDecRet H264SwDecDecode(H264SwDecInst decInst, H264SwDecInput *pInput, H264SwDecOutput *pOutput)
{
    DEC_API_TRC("H264SwDecDecode#");
    if (pInput == NULL || pOutput == NULL) return H264SWDEC_PARAM_ERR;
    if (pInput->pStream == NULL || pInput->dataLen == 0) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    if (decInst == NULL || c->stat == ST_UNINIT) return H264SWDEC_NOT_INITIALIZED;

    H264SwDecRet ret = H264SWDEC_STRM_PROCESSED;
    u32 len = pInput->dataLen;
    u8 *p = pInput->pStream;
    pOutput->pStrmCurrPos = NULL;
    c->dec.intra_conceal = (int)pInput->intraConcealmentMethod;
    c->dec.last_out_slot1 = 0;      /* H264SwDecLastPictureMbInfo / Residual: this call may decode into that picture's slot */
    do {
        int r;
        uint32_t nread = 0;
        if (c->stat == ST_NEW_HEADERS) {
            r = DEC_HDRS_RDY;
            c->stat = ST_INIT;
        } else {
            r = h264dec_decode(&c->dec, p, len, pInput->picId, &nread);
        }
        p += nread;
        len = ((int32_t)(len - nread) >= 0) ? len - nread : 0;
        pOutput->pStrmCurrPos = p;
        switch (r) {
        case DEC_HDRS_RDY:
            if (c->dec.dpb.flushed && c->dec.dpb.num_out != c->dec.dpb.out_index) {
                c->dec.dpb.flushed = 0;
                c->stat = ST_NEW_HEADERS;
                ret = H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY;
            } else {
                ret = H264SWDEC_HDRS_RDY_BUFF_NOT_EMPTY;
            }
            len = 0;
            break;
        case DEC_PIC_RDY:
            c->pic_number++;
            ret = len == 0 ? H264SWDEC_PIC_RDY : H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY;
            len = 0;
            break;
        case DEC_PARAM_SET_ERROR:
            if (!h264dec_valid_param_sets(&c->dec) && len == 0) ret = H264SWDEC_STRM_ERR;
            break;
        case DEC_MEMALLOC_ERROR:
            ret = H264SWDEC_MEMFAIL;
            len = 0;
            break;
        default:
            break;
        }
    } while (len);
    return ret;
}

H264SwDecApiVersion H264SwDecGetAPIVersion(void)
{
    H264SwDecApiVersion v;
    v.major = 2;
    v.minor = 3;
    return v;
}

H264SwDecRet H264SwDecNextPicture(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer)
{
    DEC_API_TRC("H264SwDecNextPicture#");
    if (decInst == NULL || pOutput == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    if (flushBuffer) h264dec_flush(&c->dec);
    uint32_t id, idr, em;
    const uint8_t *pic = h264dec_next_output(&c->dec, &id, &idr, &em);
    if (!pic) return H264SWDEC_OK;
    pOutput->pOutputPicture = (u32 *)(void *)pic;
    pOutput->picId = id;
    pOutput->isIdrPicture = idr;
    pOutput->nbrOfErrMBs = em;
    return H264SWDEC_PIC_RDY;
}

/* NextPicture with the picture converted to RGBA on the GPU (Decoder.js
 * `rgb: true`, DecoderPost.js:82-97 + :420-560): rgba receives
 * picWidth * picHeight * 4 bytes and pOutputPicture points to it. */
H264SwDecRet H264SwDecNextPictureRGBA(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer, u8 *rgba)
{
    if (decInst == NULL || pOutput == NULL || rgba == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    if (flushBuffer) h264dec_flush(&c->dec);
    uint32_t id, idr, em;
    const uint8_t *pic = h264dec_next_output_rgba(&c->dec, &id, &idr, &em, rgba);
    if (!pic) return H264SWDEC_OK;
    pOutput->pOutputPicture = (u32 *)(void *)pic;
    pOutput->picId = id;
    pOutput->isIdrPicture = idr;
    pOutput->nbrOfErrMBs = em;
    return H264SWDEC_PIC_RDY;
}

/* NextPicture with the picture cropped to the active SPS's crop window on
 * the GPU (DecTestBench -C, CropPicture :588-666): dst receives cropOutWidth *
 * cropOutHeight * 3 / 2 bytes of I420, or * 4 bytes of RGBA with rgba != 0
 * (the whole picture when croppingFlag == 0), and pOutputPicture points to
 * it.  A backend without read_crop: H264SWDEC_PARAM_ERR, no host fallback. */
H264SwDecRet H264SwDecNextPictureCropped(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer, u8 *dst,
                                         u32 rgba)
{
    if (decInst == NULL || pOutput == NULL || dst == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    if (!c->dec.be.read_crop) return H264SWDEC_PARAM_ERR;
    if (flushBuffer) h264dec_flush(&c->dec);
    uint32_t id, idr, em;
    const uint8_t *pic = h264dec_next_output_crop(&c->dec, &id, &idr, &em, dst, rgba != 0);
    if (!pic) return H264SWDEC_OK;
    pOutput->pOutputPicture = (u32 *)(void *)pic;
    pOutput->picId = id;
    pOutput->isIdrPicture = idr;
    pOutput->nbrOfErrMBs = em;
    return H264SWDEC_PIC_RDY;
}

/* H264SwDecNextPictureTensor (desc: an h264mi_tensor_desc), resized == 1
 * ...TensorResized (an h264mi_tensor_resize_desc) and resized == 2 ...TensorFit
 * (an h264mi_tensor_fit_desc) and resized == 3 ...TensorLayout (an
 * h264mi_tensor_layout_desc) and resized == 4 ...TensorDest (the same, into the
 * strided destination dest, which may be NULL); a window with cw == 0 is the active SPS's crop
 * window.  Everything the export can refuse is checked
 * before a picture is taken from the DPB. */
static H264SwDecRet next_picture_tensor(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                        const void *desc, int resized, const h264mi_tensor_dest *dest, void *d_dst,
                                        void *hip_stream)
{
    if (decInst == NULL || pOutput == NULL || d_dst == NULL || desc == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    /* the backend member each form runs over, by `resized` */
    const int have[5] = {c->dec.be.export_tensor != NULL, c->dec.be.export_tensor_resized != NULL,
                         c->dec.be.export_tensor_fit != NULL, c->dec.be.export_tensor_layout != NULL,
                         c->dec.be.export_tensor_dest != NULL};
    if (resized < 0 || resized > 4 || !have[resized]) return H264SWDEC_PARAM_ERR;
    h264mi_tensor_layout_desc l;
    memset(&l, 0, sizeof(l));
    if (resized >= 3) l = *(const h264mi_tensor_layout_desc *)desc;
    else if (resized == 2) l.f = *(const h264mi_tensor_fit_desc *)desc;
    else if (resized) l.f.r = *(const h264mi_tensor_resize_desc *)desc;
    else l.f.r.t = *(const h264mi_tensor_desc *)desc;
    h264mi_tensor_fit_desc *f = &l.f;
    h264mi_tensor_resize_desc *r = &f->r;
    h264mi_tensor_desc *t = &r->t;
    if (h264mi_tensor_colour_resolve(t->mode, 2, 0, 2, 2) < 0 ||
        !(resized >= 3 ? layout_desc_fixed_ok(&l) : resized == 2 ? fit_desc_fixed_ok(f)
          : resized ? resize_desc_fixed_ok(r) : tensor_desc_fixed_ok(t)) ||
        !export_aligned(d_dst, 0, export_elem_size(t->dtype)))
        return H264SWDEC_PARAM_ERR;
    /* (what dest_ok refuses whatever the window turns out to be; one picture is one item, so its clip is 1) */
    if (resized == 4 && dest && (!dest_fixed_ok(dest, l.layout == H264MI_LAYOUT_INTERLEAVED) || dest->clip != 1))
        return H264SWDEC_PARAM_ERR;
    if (flushBuffer) h264dec_flush(&c->dec);
    const Sps *s = h264dec_active_sps(&c->dec);
    if (!s) return H264SWDEC_OK;                    /* no headers yet: no picture either */
    if (t->cw == 0) {
        const export_window w = sps_crop_window(s);
        t->x = w.x; t->y = w.y; t->cw = w.cw; t->ch = w.ch;
    }
    const int width = 16 * s->w_mbs, height = 16 * s->h_mbs;
    if (!(resized >= 3 ? layout_window_ok(&l, width, height) : resized == 2 ? fit_window_ok(f, width, height, NULL)
          : resized    ? resize_window_ok(r, width, height) : tensor_window_ok(t, width, height)))
        return H264SWDEC_PARAM_ERR;
    /* (one picture is one item: dest_ok then asks for clip == 1) */
    if (resized == 4 && dest &&
        !dest_ok(dest, export_elem_size(t->dtype), H264MI_TENSOR_LAYOUT(t->mode) == H264MI_TENSOR_RGB ? 3 : 1,
                 layout_unresized(&l) ? t->ch : r->oh, layout_unresized(&l) ? t->cw : r->ow,
                 l.layout == H264MI_LAYOUT_INTERLEAVED, 1, 0))
        return H264SWDEC_PARAM_ERR;
    uint32_t id, idr, em;
    int failed = 0;
    /* (a layout descriptor starts with its fit descriptor, that with its resize descriptor, and that with its
     * h264mi_tensor_desc) */
    const uint8_t *pic = resized == 4
        ? h264dec_next_output_tensor_dest(&c->dec, &id, &idr, &em, &l, dest, d_dst, hip_stream, &failed)
        : h264dec_next_output_tensor(&c->dec, &id, &idr, &em, &l, resized, d_dst, hip_stream, &failed);
    if (failed) return H264SWDEC_PARAM_ERR;         /* (d_dst not on the decoder's GPU) */
    if (!pic) return H264SWDEC_OK;
    pOutput->pOutputPicture = (u32 *)(void *)pic;
    pOutput->picId = id;
    pOutput->isIdrPicture = idr;
    pOutput->nbrOfErrMBs = em;
    return H264SWDEC_PIC_RDY;
}

/* NextPicture with the picture exported to device memory as a planar tensor
 * (include/h264mi.h); desc == NULL: RGB fp16, scale 1/255, over the active
 * SPS's crop window.  A backend without export_tensor: H264SWDEC_PARAM_ERR, no
 * host fallback. */
H264SwDecRet H264SwDecNextPictureTensor(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                        const h264mi_tensor_desc *desc, void *d_dst, void *hip_stream)
{
    h264mi_tensor_desc t;
    memset(&t, 0, sizeof(t));
    t.mode = H264MI_TENSOR_RGB;
    t.dtype = H264MI_TENSOR_F16;
    for (int p = 0; p < 3; p++) t.scale[p] = 1.0f / 255.0f;
    return next_picture_tensor(decInst, pOutput, flushBuffer, desc ? desc : &t, 0, NULL, d_dst, hip_stream);
}

/* NextPictureTensor with the tensor resized on the GPU (include/h264mi.h) */
H264SwDecRet H264SwDecNextPictureTensorResized(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                               const h264mi_tensor_resize_desc *desc, void *d_dst, void *hip_stream)
{
    return next_picture_tensor(decInst, pOutput, flushBuffer, desc, 1, NULL, d_dst, hip_stream);
}

/* NextPictureTensorResized letterboxed (include/h264mi.h) */
H264SwDecRet H264SwDecNextPictureTensorFit(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                           const h264mi_tensor_fit_desc *desc, void *d_dst, void *hip_stream)
{
    return next_picture_tensor(decInst, pOutput, flushBuffer, desc, 2, NULL, d_dst, hip_stream);
}

/* any of the three under a layout descriptor (include/h264mi.h) */
H264SwDecRet H264SwDecNextPictureTensorLayout(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                              const h264mi_tensor_layout_desc *desc, void *d_dst, void *hip_stream)
{
    return next_picture_tensor(decInst, pOutput, flushBuffer, desc, 3, NULL, d_dst, hip_stream);
}

/* NextPictureTensorLayout into a strided destination (include/h264mi.h) */
H264SwDecRet H264SwDecNextPictureTensorDest(H264SwDecInst decInst, H264SwDecPicture *pOutput, u32 flushBuffer,
                                            const h264mi_tensor_layout_desc *desc, const h264mi_tensor_dest *dest,
                                            void *d_dst, void *hip_stream)
{
    return next_picture_tensor(decInst, pOutput, flushBuffer, desc, 4, dest, d_dst, hip_stream);
}

/* the colour id of the last tensor a call above delivered; -1: none yet */
int H264SwDecLastTensorColour(H264SwDecInst decInst)
{
    if (decInst == NULL) return -1;
    return ((DecContainer *)decInst)->dec.last_tensor_colour1 - 1;
}

/* The kept fields (decoder.h's H264_KEEP_*) behind the H264SwDecKeep* /
 * H264SwDecLastPicture* call pairs (include/h264mi.h): a field's descriptor
 * type and its two rules (common/export_desc.h).  Every field descriptor
 * starts like FieldHead; `blocks`: the window is in 4x4 blocks and absent when
 * its width is 0 (then: the blocks covering the crop window), else it is in
 * luma samples and absent when width and height are 0 (then: the crop window). */
typedef struct { int x, y, cw, ch, count, dtype; } FieldHead;
typedef union {
    FieldHead head;
    h264mi_mbinfo_desc mbinfo;
    h264mi_residual_desc residual;
    h264mi_accmv_desc accmv;
} FieldDesc;

static int mbinfo_fixed(const FieldDesc *d) { return mbinfo_desc_fixed_ok(&d->mbinfo); }
static int mbinfo_window(const FieldDesc *d, int w_mbs, int h_mbs) { return mbinfo_window_ok(&d->mbinfo, w_mbs, h_mbs); }
static int residual_fixed(const FieldDesc *d) { return residual_desc_fixed_ok(&d->residual); }
static int residual_window(const FieldDesc *d, int w_mbs, int h_mbs) { return residual_window_ok(&d->residual, w_mbs, h_mbs); }
static int accmv_fixed(const FieldDesc *d) { return accmv_desc_fixed_ok(&d->accmv); }
static int accmv_window(const FieldDesc *d, int w_mbs, int h_mbs) { return accmv_window_ok(&d->accmv, w_mbs, h_mbs); }

static const struct {
    size_t size;
    int (*fixed_ok)(const FieldDesc *d);
    int (*window_ok)(const FieldDesc *d, int w_mbs, int h_mbs);
    int blocks;
} field_rules[H264_KEEP_KINDS] = {
    [H264_KEEP_RECORDS] = {sizeof(h264mi_mbinfo_desc), mbinfo_fixed, mbinfo_window, 1},
    [H264_KEEP_COEFS] = {sizeof(h264mi_residual_desc), residual_fixed, residual_window, 0},
    [H264_KEEP_ACCMV] = {sizeof(h264mi_accmv_desc), accmv_fixed, accmv_window, 0},
};

/* Retention of a kind for its H264SwDecLastPicture* call: the backend keeps it
 * across configure, so it may be called before the headers */
static H264SwDecRet keep_field(H264SwDecInst decInst, int kind, u32 on)
{
    if (decInst == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    if (!c->dec.be.field[kind].keep || !c->dec.be.field[kind].export_field) return H264SWDEC_PARAM_ERR;
    if (c->dec.be.field[kind].keep(c->dec.be.ctx, kind, on != 0)) return H264SWDEC_PARAM_ERR;
    c->dec.keep[kind] = on != 0;
    return H264SWDEC_OK;
}

/* The field of a kind of the picture the last H264SwDecNextPicture* call
 * delivered.  The DPB is not touched.  Everything the export can refuse is
 * checked before anything is queued. */
static H264SwDecRet last_picture_field(H264SwDecInst decInst, int kind, const void *desc, void *d_dst, void *hip_stream)
{
    if (decInst == NULL || desc == NULL || d_dst == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    if (!c->dec.be.field[kind].export_field || !c->dec.keep[kind]) return H264SWDEC_PARAM_ERR;
    FieldDesc m;
    memcpy(&m, desc, field_rules[kind].size);
    if (!field_rules[kind].fixed_ok(&m) || !export_aligned(d_dst, 0, export_elem_size(m.head.dtype))) return H264SWDEC_PARAM_ERR;
    const Sps *s = h264dec_active_sps(&c->dec);
    if (!s || !c->dec.last_out_slot1) return H264SWDEC_OK;      /* no picture delivered */
    if (m.head.cw == 0 && (field_rules[kind].blocks || m.head.ch == 0)) {
        export_window w = sps_crop_window(s);
        if (field_rules[kind].blocks) w = export_window_blocks(w);
        m.head.x = w.x; m.head.y = w.y; m.head.cw = w.cw; m.head.ch = w.ch;
    }
    if (!field_rules[kind].window_ok(&m, s->w_mbs, s->h_mbs)) return H264SWDEC_PARAM_ERR;
    if (c->dec.be.field[kind].export_field(c->dec.be.ctx, kind, c->dec.last_out_slot1 - 1, &m, d_dst, hip_stream))
        return H264SWDEC_PARAM_ERR;         /* (d_dst not on the decoder's GPU) */
    return H264SWDEC_PIC_RDY;
}

/* Record retention and the MB side-information field; desc->bw == 0: the
 * blocks covering the active SPS's crop window */
H264SwDecRet H264SwDecKeepMbInfo(H264SwDecInst decInst, u32 on) { return keep_field(decInst, H264_KEEP_RECORDS, on); }

H264SwDecRet H264SwDecLastPictureMbInfo(H264SwDecInst decInst, const h264mi_mbinfo_desc *desc, void *d_dst,
                                        void *hip_stream)
{
    return last_picture_field(decInst, H264_KEEP_RECORDS, desc, d_dst, hip_stream);
}

/* Coefficient retention and the residual; desc->cw == desc->ch == 0: the active SPS's crop window */
H264SwDecRet H264SwDecKeepResidual(H264SwDecInst decInst, u32 on) { return keep_field(decInst, H264_KEEP_COEFS, on); }

H264SwDecRet H264SwDecLastPictureResidual(H264SwDecInst decInst, const h264mi_residual_desc *desc, void *d_dst,
                                          void *hip_stream)
{
    return last_picture_field(decInst, H264_KEEP_COEFS, desc, d_dst, hip_stream);
}

/* Origin-map retention and the accumulated motion; desc->cw == desc->ch == 0: the active SPS's crop window */
H264SwDecRet H264SwDecKeepAccMotion(H264SwDecInst decInst, u32 on) { return keep_field(decInst, H264_KEEP_ACCMV, on); }

H264SwDecRet H264SwDecLastPictureAccMotion(H264SwDecInst decInst, const h264mi_accmv_desc *desc, void *d_dst,
                                           void *hip_stream)
{
    return last_picture_field(decInst, H264_KEEP_ACCMV, desc, d_dst, hip_stream);
}

/* The accumulated motion resized: H264SwDecLastPictureAccMotion's steps with
 * the resize descriptor's two rules and the backend's member for it (the
 * resized export has no row in field_rules: it keeps nothing of its own) */
H264SwDecRet H264SwDecLastPictureAccMotionResized(H264SwDecInst decInst, const h264mi_accmv_resize_desc *desc,
                                                  void *d_dst, void *hip_stream)
{
    if (decInst == NULL || desc == NULL || d_dst == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    if (!c->dec.be.export_accmv_resized || !c->dec.keep[H264_KEEP_ACCMV]) return H264SWDEC_PARAM_ERR;
    h264mi_accmv_resize_desc m = *desc;
    if (!accmv_resize_fixed_ok(&m) || !export_aligned(d_dst, 0, export_elem_size(m.f.dtype))) return H264SWDEC_PARAM_ERR;
    const Sps *s = h264dec_active_sps(&c->dec);
    if (!s || !c->dec.last_out_slot1) return H264SWDEC_OK;      /* no picture delivered */
    if (m.f.cw == 0 && m.f.ch == 0) {
        const export_window w = sps_crop_window(s);
        m.f.x = w.x; m.f.y = w.y; m.f.cw = w.cw; m.f.ch = w.ch;
    }
    if (!accmv_resize_window_ok(&m, s->w_mbs, s->h_mbs)) return H264SWDEC_PARAM_ERR;
    if (c->dec.be.export_accmv_resized(c->dec.be.ctx, c->dec.last_out_slot1 - 1, &m, d_dst, hip_stream))
        return H264SWDEC_PARAM_ERR;         /* (d_dst not on the decoder's GPU) */
    return H264SWDEC_PIC_RDY;
}

/* Boxes of the delivered picture as resized tensors (include/h264mi.h): like
 * the call above a LastPicture call over one backend member, and it needs no
 * retention (the frame slot is there until the next decode).  Box coordinates
 * are the delivered window's: the SPS crop offset is added here, and
 * H264MI_TENSOR_COLOUR_STREAM resolves from the delivered picture's VUI and the
 * crop window's size, as the whole-picture tensor's does.  fit != NULL (desc
 * = &fit->r): every box letterboxed into the canvas; lay != NULL (fit =
 * &lay->f): under its layout, through the backend's member for that. */
static H264SwDecRet last_picture_rois(H264SwDecInst decInst, const h264mi_tensor_resize_desc *desc,
                                      const h264mi_tensor_fit_desc *fit, const h264mi_tensor_layout_desc *lay,
                                      const h264mi_roi *rois, u32 nrois, void *d_dst, void *hip_stream)
{
    if (decInst == NULL || desc == NULL || rois == NULL || d_dst == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    if (!(lay ? c->dec.be.export_tensor_layout != NULL : fit ? c->dec.be.export_tensor_rois_fit != NULL
                                                            : c->dec.be.export_tensor_rois != NULL))
        return H264SWDEC_PARAM_ERR;
    /* (without fit: desc stretched, which has rois_ok's rules) */
    h264mi_tensor_layout_desc ml;
    memset(&ml, 0, sizeof(ml));
    if (lay) ml = *lay;
    else if (fit) ml.f = *fit;
    else ml.f.r = *desc;
    h264mi_tensor_fit_desc *mf = &ml.f;
    h264mi_tensor_resize_desc *m = &mf->r;
    if (nrois < 1 || nrois > 0x7FFFFFFF / sizeof(h264mi_roi) || h264mi_tensor_colour_resolve(m->t.mode, 2, 0, 2, 2) < 0 ||
        !(lay ? layout_desc_fixed_ok(&ml) && !layout_unresized(&ml) : fit_desc_fixed_ok(mf)) ||
        (m->t.x | m->t.y | m->t.cw | m->t.ch) ||
        !export_aligned(d_dst, 0, export_elem_size(m->t.dtype)))
        return H264SWDEC_PARAM_ERR;
    for (u32 k = 0; k < nrois; k++)
        if (rois[k].pic != 0) return H264SWDEC_PARAM_ERR;
    const Sps *s = h264dec_active_sps(&c->dec);
    if (!s || !c->dec.last_out_slot1) return H264SWDEC_OK;      /* no picture delivered */
    const export_window w = sps_crop_window(s);
    h264mi_roi *b = (h264mi_roi *)malloc(nrois * sizeof(*b));
    if (!b) return H264SWDEC_MEMFAIL;
    int ok = 1;
    for (u32 k = 0; k < nrois && ok; k++) {
        b[k] = rois[k];
        ok = b[k].x >= 0 && b[k].y >= 0 && b[k].cw >= 1 && b[k].ch >= 1 && b[k].cw <= w.cw - b[k].x &&
             b[k].ch <= w.ch - b[k].y;
        if (ok) { b[k].x += w.x; b[k].y += w.y; }
    }
    ok = ok && rois_fit_ok(mf, b, (int)nrois, 1, 16 * s->w_mbs, 16 * s->h_mbs);
    const int colour = h264mi_tensor_colour_resolve(m->t.mode, c->dec.last_out_vui_matrix, c->dec.last_out_vui_full, w.cw, w.ch);
    if (H264MI_TENSOR_LAYOUT(m->t.mode) == H264MI_TENSOR_RGB) m->t.mode = H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, colour, 0);
    /* (a failure of the export itself: d_dst not on the decoder's GPU) */
    ok = ok && !(lay ? c->dec.be.export_tensor_layout(c->dec.be.ctx, c->dec.last_out_slot1 - 1, &ml, b, (int)nrois, d_dst,
                                                      hip_stream)
                 : fit ? c->dec.be.export_tensor_rois_fit(c->dec.be.ctx, c->dec.last_out_slot1 - 1, mf, b, (int)nrois, d_dst,
                                                        hip_stream)
                     : c->dec.be.export_tensor_rois(c->dec.be.ctx, c->dec.last_out_slot1 - 1, m, b, (int)nrois, d_dst,
                                                    hip_stream));
    free(b);
    if (!ok) return H264SWDEC_PARAM_ERR;
    c->dec.last_tensor_colour1 = colour + 1;
    return H264SWDEC_PIC_RDY;
}

H264SwDecRet H264SwDecLastPictureTensorRois(H264SwDecInst decInst, const h264mi_tensor_resize_desc *desc,
                                            const h264mi_roi *rois, u32 nrois, void *d_dst, void *hip_stream)
{
    return last_picture_rois(decInst, desc, NULL, NULL, rois, nrois, d_dst, hip_stream);
}

/* the same, every box letterboxed into the canvas (include/h264mi.h) */
H264SwDecRet H264SwDecLastPictureTensorRoisFit(H264SwDecInst decInst, const h264mi_tensor_fit_desc *desc,
                                               const h264mi_roi *rois, u32 nrois, void *d_dst, void *hip_stream)
{
    return last_picture_rois(decInst, desc ? &desc->r : NULL, desc, NULL, rois, nrois, d_dst, hip_stream);
}

/* the same under a layout descriptor (include/h264mi.h) */
H264SwDecRet H264SwDecLastPictureTensorRoisLayout(H264SwDecInst decInst, const h264mi_tensor_layout_desc *desc,
                                                  const h264mi_roi *rois, u32 nrois, void *d_dst, void *hip_stream)
{
    return last_picture_rois(decInst, desc ? &desc->f.r : NULL, desc ? &desc->f : NULL, desc, rois, nrois, d_dst,
                             hip_stream);
}

/* Affine warps of the delivered picture (include/h264mi.h): a LastPicture call
 * like the boxes above.  The window the taps are confined to is the SPS crop
 * window (desc->t.cw == 0) or a window inside it, in its coordinates: the crop
 * offset goes onto the window and the matrices stay as they are (they map into
 * the window), so no tap reaches the MB-aligned picture's padding.  STREAM
 * resolves as for the boxes, by size from the crop window. */
H264SwDecRet H264SwDecLastPictureTensorWarps(H264SwDecInst decInst, const h264mi_tensor_warp_desc *desc,
                                             const h264mi_warp *warps, u32 nwarps, void *d_dst, void *hip_stream)
{
    if (decInst == NULL || desc == NULL || warps == NULL || d_dst == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    if (!c->dec.be.export_tensor_warps) return H264SWDEC_PARAM_ERR;
    h264mi_tensor_warp_desc m = *desc;
    if (nwarps < 1 || nwarps > 0x7FFFFFFF / sizeof(h264mi_warp) || h264mi_tensor_colour_resolve(m.t.mode, 2, 0, 2, 2) < 0 ||
        !warp_desc_fixed_ok(&m) || !export_aligned(d_dst, 0, export_elem_size(m.t.dtype)) || !warps_ok(warps, (int)nwarps, 1))
        return H264SWDEC_PARAM_ERR;
    const Sps *s = h264dec_active_sps(&c->dec);
    if (!s || !c->dec.last_out_slot1) return H264SWDEC_OK;      /* no picture delivered */
    const export_window w = sps_crop_window(s);
    if (m.t.cw == 0) {
        m.t.x = w.x; m.t.y = w.y; m.t.cw = w.cw; m.t.ch = w.ch;
    } else {
        if (m.t.x < 0 || m.t.y < 0 || m.t.cw < 1 || m.t.ch < 1 || m.t.cw > w.cw - m.t.x || m.t.ch > w.ch - m.t.y)
            return H264SWDEC_PARAM_ERR;
        m.t.x += w.x; m.t.y += w.y;
    }
    if (!warp_window_ok(&m, 16 * s->w_mbs, 16 * s->h_mbs)) return H264SWDEC_PARAM_ERR;
    const int colour = h264mi_tensor_colour_resolve(m.t.mode, c->dec.last_out_vui_matrix, c->dec.last_out_vui_full, w.cw, w.ch);
    if (H264MI_TENSOR_LAYOUT(m.t.mode) == H264MI_TENSOR_RGB) m.t.mode = H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, colour, 0);
    /* (a failure of the export itself: d_dst not on the decoder's GPU) */
    if (c->dec.be.export_tensor_warps(c->dec.be.ctx, c->dec.last_out_slot1 - 1, &m, warps, (int)nwarps, d_dst, hip_stream))
        return H264SWDEC_PARAM_ERR;
    c->dec.last_tensor_colour1 = colour + 1;
    return H264SWDEC_PIC_RDY;
}

/* Statistics of the delivered picture (include/h264mi.h): a
 * LastPicture call like the boxes above, over the backend's export_stats.
 * Without boxes the window is the SPS crop window (desc->cw == 0) or a window
 * inside it, in its coordinates; boxes are in its coordinates too: the crop
 * offset is added here.  H264MI_TENSOR_COLOUR_STREAM (RGB) is taken out of the
 * descriptor ahead of the rules, which know ids only, and resolves from the
 * delivered picture's VUI (BT.601 where it names no matrix).  No reference
 * picture: the decoder does not hold the previously delivered slot. */
H264SwDecRet H264SwDecLastPictureStats(H264SwDecInst decInst, const h264mi_stats_desc *desc, const h264mi_roi *rois,
                                       u32 nrois, void *d_dst, void *hip_stream)
{
    if (decInst == NULL || desc == NULL || d_dst == NULL) return H264SWDEC_PARAM_ERR;
    DecContainer *c = (DecContainer *)decInst;
    if (!c->dec.be.export_stats) return H264SWDEC_PARAM_ERR;
    h264mi_stats_desc m = *desc;
    const int from_stream = m.planes == H264MI_STATS_RGB && m.colour == H264MI_TENSOR_COLOUR_STREAM;
    if (from_stream) m.colour = 0;
    if ((rois ? nrois < 1 || nrois > 0x7FFFFFFF / sizeof(h264mi_roi) || (m.x | m.y | m.cw | m.ch) : nrois != 0) ||
        !stats_desc_fixed_ok(&m) || !export_aligned(d_dst, 0, 8))
        return H264SWDEC_PARAM_ERR;
    for (u32 k = 0; rois && k < nrois; k++)
        if (rois[k].pic != 0) return H264SWDEC_PARAM_ERR;
    const Sps *s = h264dec_active_sps(&c->dec);
    if (!s || !c->dec.last_out_slot1) return H264SWDEC_OK;      /* no picture delivered */
    const export_window w = sps_crop_window(s);
    h264mi_roi *b = NULL;
    int ok = 1;
    if (rois) {
        b = (h264mi_roi *)malloc(nrois * sizeof(*b));
        if (!b) return H264SWDEC_MEMFAIL;
        for (u32 k = 0; k < nrois && ok; k++) {
            b[k] = rois[k];
            ok = stats_box_ok(b[k].x, b[k].y, b[k].cw, b[k].ch, w.cw, w.ch);
            if (ok) { b[k].x += w.x; b[k].y += w.y; }
        }
        ok = ok && stats_rois_ok(&m, b, (int)nrois, 1, 16 * s->w_mbs, 16 * s->h_mbs);
    } else {
        if (m.cw == 0) {
            ok = !(m.x | m.y | m.ch);
            m.cw = w.cw; m.ch = w.ch;
        }
        ok = ok && stats_window_ok(&m, w.cw, w.ch);
        if (ok) { m.x += w.x; m.y += w.y; }
        ok = ok && stats_window_ok(&m, 16 * s->w_mbs, 16 * s->h_mbs);
    }
    const int colour = from_stream ? h264mi_tensor_colour_resolve(H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_STREAM,
                                                                                     H264MI_TENSOR_UNSPEC_BT601),
                                                                  c->dec.last_out_vui_matrix, c->dec.last_out_vui_full, w.cw, w.ch)
                                   : m.colour;
    m.colour = colour;
    /* (a failure of the export itself: d_dst not on the decoder's GPU) */
    ok = ok && !c->dec.be.export_stats(c->dec.be.ctx, c->dec.last_out_slot1 - 1, &m, b, rois ? (int)nrois : 0, d_dst, hip_stream);
    free(b);
    if (!ok) return H264SWDEC_PARAM_ERR;
    c->dec.last_tensor_colour1 = colour + 1;
    return H264SWDEC_PIC_RDY;
}

H264SwDecRet H264SwDecGetTiming(H264SwDecInst decInst, double *parse_s, double *submit_s, double *wait_s,
                                double *copy_s, u32 *pictures)
{
    if (decInst == NULL) return H264SWDEC_PARAM_ERR;
    const DecContainer *c = (const DecContainer *)decInst;
    if (parse_s) *parse_s = c->dec.t_parse;
    if (submit_s) *submit_s = c->dec.t_submit;
    if (wait_s) *wait_s = c->dec.t_wait;
    if (copy_s) *copy_s = c->dec.t_copy;
    if (pictures) *pictures = (u32)c->dec.n_output;
    return H264SWDEC_OK;
}

/* ------------------------------------------------------------------------ */
/* wasm / JS glue (Decoder.c): one global instance per process               */
/* ------------------------------------------------------------------------ */
static H264SwDecInst g_inst;
static H264SwDecInput g_in;
static H264SwDecOutput g_out;
static H264SwDecPicture g_pic;
static H264SwDecInfo g_info;
static u32 g_pic_decode, g_pic_display;
static struct { u32 length; u8 *buffer; } g_stream;
static broadway_headers_cb g_on_headers;
static broadway_picture_cb g_on_picture;
static void *g_user;

void broadwaySetCallbacks(broadway_headers_cb on_headers, broadway_picture_cb on_picture, void *user)
{
    g_on_headers = on_headers;
    g_on_picture = on_picture;
    g_user = user;
}

u32 broadwayInit(void)
{
    if (H264SwDecInit(&g_inst, 0) != H264SWDEC_OK) {
        fprintf(stderr, "DECODER INITIALIZATION FAILED\n");
        broadwayExit();
        return (u32)-1;
    }
    g_pic_decode = g_pic_display = 1;
    return 0;
}

u8 *broadwayCreateStream(u32 length)
{
    free(g_stream.buffer);
    g_stream.buffer = (u8 *)malloc(length ? length : 1);
    g_stream.length = length;
    return g_stream.buffer;
}

static u32 broadway_decode(void)
{
    g_in.picId = g_pic_decode;
    H264SwDecRet ret = H264SwDecDecode(g_inst, &g_in, &g_out);
    switch ((int)ret) {
    case H264SWDEC_HDRS_RDY_BUFF_NOT_EMPTY:
        if (H264SwDecGetInfo(g_inst, &g_info) != H264SWDEC_OK) return (u32)-1;
        if (g_on_headers) g_on_headers(g_user);
        g_in.dataLen -= (u32)(g_out.pStrmCurrPos - g_in.pStream);
        g_in.pStream = g_out.pStrmCurrPos;
        break;
    case H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY:
        g_in.dataLen -= (u32)(g_out.pStrmCurrPos - g_in.pStream);
        g_in.pStream = g_out.pStrmCurrPos;
        /* fall through */
    case H264SWDEC_PIC_RDY:
        g_in.dataLen = 0;           /* Decoder.c:130: rest of the buffer is dropped */
        g_pic_decode++;
        while (H264SwDecNextPicture(g_inst, &g_pic, 0) == H264SWDEC_PIC_RDY) {
            g_pic_display++;
            if (g_on_picture) g_on_picture(g_user, (u8 *)g_pic.pOutputPicture, g_info.picWidth, g_info.picHeight);
        }
        break;
    case H264SWDEC_STRM_PROCESSED:
    case H264SWDEC_STRM_ERR:
        g_in.dataLen = 0;
        break;
    default:
        break;
    }
    return (u32)ret;
}

void broadwayPlayStream(u32 length)
{
    g_stream.length = length;
    g_in.pStream = g_stream.buffer;
    g_in.dataLen = length;
    do {
        broadway_decode();
    } while (g_in.dataLen > 0);
}

void broadwayExit(void)
{
    if (g_inst) H264SwDecRelease(g_inst);
    g_inst = NULL;
    free(g_stream.buffer);
    g_stream.buffer = NULL;
}

u32 broadwayGetMajorVersion(void) { return H264SwDecGetAPIVersion().major; }
u32 broadwayGetMinorVersion(void) { return H264SwDecGetAPIVersion().minor; }
