/* Host side of the resized H264SwDec tensor calls under H264MI_RESIZE_BICUBIC
 * (DESIGN 3.5o), with no GPU: the product host path (api.c, decoder.c, dpb.c,
 * hipback.cpp) on the CPU stand-in of the engine (oracle/null_device.cpp),
 * which has no export.  The engine exports defined here launch nothing; each
 * records the filter and the size it is handed.  tests/test_bicubic_cpu.py
 * builds this with AddressSanitizer + UBSan, runs it and reads its lines:
 *   before resized <ret> fit <ret> layout <ret> rois <ret> rois_fit <ret> rois_layout <ret>
 *   before_bad <filter> resized <ret> fit <ret> layout <ret> rois <ret> rois_fit <ret> rois_layout <ret>
 *   pic <k> form <f> ret <ret> calls <n> filter <filter> size <ow>,<oh>
 *   box <k> form <f> ret <ret> calls <n> filter <filter> size <ow>,<oh>
 *   refused <bad calls refused without reaching the engine> of <bad calls> then <pictures delivered>
 */
#include "../include/h264mi.h"
#include "../broadway_amd/csrc/gen/h264gen.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_calls;
static h264mi_tensor_resize_desc g_desc;

#define UNUSED_PICS (void)e, (void)n, (void)streams, (void)slots, (void)d_out, (void)out_stride, (void)hip_stream

int h264mi_engine_export_tensor_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                        const h264mi_tensor_resize_desc *desc, void *d_out, size_t out_stride,
                                        void *hip_stream)
{
    UNUSED_PICS;
    g_calls++;
    g_desc = *desc;
    return 0;
}

int h264mi_engine_export_tensor_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                                    const h264mi_tensor_fit_desc *desc, void *d_out, size_t out_stride, void *hip_stream)
{
    UNUSED_PICS;
    g_calls++;
    g_desc = desc->r;
    return 0;
}

int h264mi_engine_export_tensor_rois(h264mi_engine *e, int n, const int *streams, const int *slots,
                                     const h264mi_tensor_resize_desc *desc, const h264mi_roi *rois, int nrois,
                                     void *d_out, size_t out_stride, void *hip_stream)
{
    UNUSED_PICS; (void)rois; (void)nrois;
    g_calls++;
    g_desc = *desc;
    return 0;
}

int h264mi_engine_export_tensor_rois_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                                         const h264mi_tensor_fit_desc *desc, const h264mi_roi *rois, int nrois,
                                         void *d_out, size_t out_stride, void *hip_stream)
{
    UNUSED_PICS; (void)rois; (void)nrois;
    g_calls++;
    g_desc = desc->r;
    return 0;
}

int h264mi_engine_export_tensor_layout(h264mi_engine *e, int n, const int *streams, const int *slots,
                                       const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois, int nrois,
                                       void *d_out, size_t out_stride, void *hip_stream)
{
    UNUSED_PICS; (void)rois; (void)nrois;
    g_calls++;
    g_desc = desc->f.r;
    return 0;
}

static uint64_t g_dst[4];       /* "device" memory no export writes */

/* the delivered (crop) window is 86 x 52: 6 x 4 is within 16 : 1 on both axes (86 <= 96, 52 <= 64).  The window is
 * left to the picture calls (cw == 0) and reserved for the box calls */
static h264mi_tensor_layout_desc good_desc(int filter)
{
    h264mi_tensor_layout_desc d;
    memset(&d, 0, sizeof(d));
    d.f.r.t.mode = H264MI_TENSOR_RGB;
    d.f.r.t.dtype = H264MI_TENSOR_F16;
    d.f.r.ow = 6; d.f.r.oh = 4; d.f.r.filter = filter;
    d.layout = H264MI_LAYOUT_INTERLEAVED;
    return d;
}

/* in the delivered window: the whole of it, and 4 x 4 flush with its far corner */
static const h264mi_roi kGood[2] = {{0, 0, 0, 86, 52}, {0, 82, 48, 4, 4}};

/* form 0: ...TensorResized / ...TensorRois; 1: ...Fit / ...RoisFit; 2: ...Layout / ...RoisLayout */
static H264SwDecRet next(H264SwDecInst inst, int form, u32 flush, const h264mi_tensor_layout_desc *d)
{
    H264SwDecPicture pic;
    return form == 0   ? H264SwDecNextPictureTensorResized(inst, &pic, flush, &d->f.r, g_dst, NULL)
           : form == 1 ? H264SwDecNextPictureTensorFit(inst, &pic, flush, &d->f, g_dst, NULL)
                       : H264SwDecNextPictureTensorLayout(inst, &pic, flush, d, g_dst, NULL);
}

static H264SwDecRet last(H264SwDecInst inst, int form, const h264mi_tensor_layout_desc *d, const h264mi_roi *rois)
{
    return form == 0   ? H264SwDecLastPictureTensorRois(inst, &d->f.r, rois, 2, g_dst, NULL)
           : form == 1 ? H264SwDecLastPictureTensorRoisFit(inst, &d->f, rois, 2, g_dst, NULL)
                       : H264SwDecLastPictureTensorRoisLayout(inst, d, rois, 2, g_dst, NULL);
}

static void print_before(const char *what, H264SwDecInst inst, int filter)
{
    const h264mi_tensor_layout_desc d = good_desc(filter);
    printf("%s resized %d fit %d layout %d rois %d rois_fit %d rois_layout %d\n", what, next(inst, 0, 0, &d),
           next(inst, 1, 0, &d), next(inst, 2, 0, &d), last(inst, 0, &d, kGood), last(inst, 1, &d, kGood),
           last(inst, 2, &d, kGood));
}

/* what a delivered picture refuses under the bicubic filter and the triangle takes, and the filters that do not
 * exist: PARAM_ERR without reaching the engine (and without taking a picture) */
static int bad_calls(H264SwDecInst inst, int *tried, int pictures)
{
    int refused = 0;
    const int calls = g_calls;
    static const int kBadFilter[3] = {1, -1, 3};
    for (int form = 0; form < 3; form++) {
        h264mi_tensor_layout_desc d;
        for (int k = 0; k < 3; k++) {
            d = good_desc(kBadFilter[k]);
            if (pictures) { (*tried)++; refused += next(inst, form, 0, &d) == H264SWDEC_PARAM_ERR && g_calls == calls; }
            else { (*tried)++; refused += last(inst, form, &d, kGood) == H264SWDEC_PARAM_ERR && g_calls == calls; }
        }
        d = good_desc(H264MI_RESIZE_BICUBIC);
        d.f.r.ow = 5;                                   /* 86 columns to 5: beyond 16 : 1 */
        (*tried)++;
        refused += (pictures ? next(inst, form, 0, &d) : last(inst, form, &d, kGood)) == H264SWDEC_PARAM_ERR &&
                   g_calls == calls;
        d = good_desc(H264MI_RESIZE_BICUBIC);
        d.f.r.oh = 3;                                   /* 52 rows to 3 */
        (*tried)++;
        refused += (pictures ? next(inst, form, 0, &d) : last(inst, form, &d, kGood)) == H264SWDEC_PARAM_ERR &&
                   g_calls == calls;
    }
    /* the unresized form of the layout descriptor has no filter */
    if (pictures) {
        h264mi_tensor_layout_desc d = good_desc(H264MI_RESIZE_BICUBIC);
        d.f.r.ow = d.f.r.oh = 0;
        (*tried)++;
        refused += next(inst, 2, 0, &d) == H264SWDEC_PARAM_ERR && g_calls == calls;
    }
    return refused;
}

int main(void)
{
    /* the crop_ltrb_6x4 geometry of tests/golden/crop.json */
    GenParams p;
    uint8_t *s = NULL;
    size_t n = 0;
    if (h264gen_preset(&p, 2, 61)) return 3;
    p.nframes = 4; p.w_mbs = 6; p.h_mbs = 4; p.slices = 2; p.gop = 3;
    p.crop_left = 6; p.crop_right = 4; p.crop_top = 2; p.crop_bottom = 10;
    p.poc_type = 2;
    if (h264gen_generate(&p, &s, &n)) return 3;

    H264SwDecInst inst;
    if (H264SwDecInit(&inst, 0) != H264SWDEC_OK) return 1;
    print_before("before", inst, H264MI_RESIZE_BICUBIC);
    printf("before_bad 1 "); print_before("", inst, 1);
    printf("before_bad -1 "); print_before("", inst, -1);
    printf("before_bad 3 "); print_before("", inst, 3);

    H264SwDecInput in;
    H264SwDecOutput out;
    memset(&in, 0, sizeof(in));
    in.pStream = s;
    in.dataLen = (u32)n;
    int pics = 0, tried = 0, refused = 0, done = 0;
    u32 pic_id = 0;
    while (!done) {
        u32 flush = 0;
        H264SwDecRet r = H264SWDEC_PIC_RDY;
        if (in.dataLen > 0) {
            in.picId = pic_id;
            r = H264SwDecDecode(inst, &in, &out);
            const u32 used = (u32)(out.pStrmCurrPos - in.pStream);
            if (used == 0 && r < 0) break;
            in.dataLen -= used;
            in.pStream = out.pStrmCurrPos;
            if (r == H264SWDEC_PIC_RDY || r == H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY) pic_id++;
        } else {
            flush = 1;
            done = 1;
        }
        if (r != H264SWDEC_PIC_RDY && r != H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY) continue;
        for (;;) {
            refused += bad_calls(inst, &tried, 1);
            const int form = pics % 3;
            /* (the last picture under the triangle, with a window only it takes: 86 columns to 5) */
            h264mi_tensor_layout_desc d = good_desc(pics == 3 ? H264MI_RESIZE_TRIANGLE : H264MI_RESIZE_BICUBIC);
            if (pics == 3) d.f.r.ow = 5;
            memset(&g_desc, 0xFF, sizeof(g_desc));
            const H264SwDecRet g = next(inst, form, flush, &d);
            if (g != H264SWDEC_PIC_RDY) break;
            flush = 0;
            printf("pic %d form %d ret %d calls %d filter %d size %d,%d\n", pics, form, g, g_calls, g_desc.filter,
                   g_desc.ow, g_desc.oh);
            refused += bad_calls(inst, &tried, 0);
            memset(&g_desc, 0xFF, sizeof(g_desc));
            const H264SwDecRet b = last(inst, form, &d, kGood);
            printf("box %d form %d ret %d calls %d filter %d size %d,%d\n", pics, form, b, g_calls, g_desc.filter,
                   g_desc.ow, g_desc.oh);
            pics++;
        }
    }
    printf("refused %d of %d then %d\n", refused, tried, pics);
    H264SwDecRelease(inst);
    h264gen_free(s);
    return 0;
}
