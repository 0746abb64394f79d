/* Host side of H264SwDecNextPictureTensorLayout and
 * H264SwDecLastPictureTensorRoisLayout, with no GPU: the product
 * host path (api.c, decoder.c, dpb.c, hipback.cpp) on the CPU stand-in of the
 * engine (oracle/null_device.cpp), which has no export.  The engine exports
 * defined here launch nothing; the layout one records what it is handed.
 * tests/test_layout_host.py builds this with AddressSanitizer + UBSan, runs it
 * and reads its lines:
 *   before next <ret> mirrored <ret> rois <ret> mirrored <ret> bad_next <ret> bad_rois <ret>
 *   pic <k> ret <ret> calls <n> colour <id> mode <hex> layout <l> fit <f> size <ow>,<oh> win <x>,<y>,<cw>,<ch>
 *       pad <r>,<g>,<b> nrois <n> stride <bytes>
 *   box <k> ret <ret> calls <n> colour <id> mode <hex> layout <l> fit <f> size <ow>,<oh> win <x>,<y>,<cw>,<ch>
 *       pad <r>,<g>,<b> nrois <n> stride <bytes> boxes <pic>,<x>,<y>,<cw>,<ch> ...
 *   refused <bad calls refused without reaching the engine> of <bad calls> then <pictures delivered>
 */
#include "../include/h264mi.h"
#include "../broadway_amd/csrc/gen/h264gen.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_calls, g_nrois, g_n;
static size_t g_stride;
static h264mi_tensor_layout_desc g_desc;
static h264mi_roi g_rois[4];

int h264mi_engine_export_tensor_layout(h264mi_engine *e, int n, const int *streams, const int *slots,
                                       const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois, int nrois,
                                       void *d_out, size_t out_stride, void *hip_stream)
{
    (void)e; (void)streams; (void)slots; (void)d_out; (void)hip_stream;
    g_calls++;
    g_desc = *desc;
    g_n = n;
    g_nrois = nrois;
    g_stride = out_stride;
    for (int k = 0; rois && k < nrois && k < 4; k++) g_rois[k] = rois[k];
    return 0;
}

/* the calls the two mirror, for their return codes before any delivery */
int h264mi_engine_export_tensor_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                                    const h264mi_tensor_fit_desc *desc, void *d_out, size_t out_stride, void *hip_stream)
{
    (void)e; (void)n; (void)streams; (void)slots; (void)desc; (void)d_out; (void)out_stride; (void)hip_stream;
    return 0;
}

int h264mi_engine_export_tensor_rois_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                                         const h264mi_tensor_fit_desc *desc, const h264mi_roi *rois, int nrois,
                                         void *d_out, size_t out_stride, void *hip_stream)
{
    (void)e; (void)n; (void)streams; (void)slots; (void)desc; (void)rois; (void)nrois; (void)d_out; (void)out_stride;
    (void)hip_stream;
    return 0;
}

static uint64_t g_dst[4];       /* "device" memory no export writes */

/* form 0: unresized; 1: stretched into 9 x 7; 2: letterboxed into 9 x 7.  The window is left to the call (cw == 0) */
static h264mi_tensor_layout_desc good_desc(int form)
{
    h264mi_tensor_layout_desc d;
    memset(&d, 0, sizeof(d));
    d.f.r.t.mode = H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_STREAM, H264MI_TENSOR_UNSPEC_BT601);
    d.f.r.t.dtype = H264MI_TENSOR_F16;
    d.layout = H264MI_LAYOUT_INTERLEAVED;
    if (form) { d.f.r.ow = 9; d.f.r.oh = 7; d.f.r.filter = H264MI_RESIZE_TRIANGLE; }
    if (form == 2) { d.f.fit = H264MI_FIT_LETTERBOX; d.f.pad[0] = 114; d.f.pad[1] = 7; d.f.pad[2] = 250; }
    return d;
}

/* in the delivered window, 86 x 52: the whole of it, and 4 x 4 flush with its far corner */
static const h264mi_roi kGood[2] = {{0, 0, 0, 86, 52}, {0, 82, 48, 4, 4}};

static void print_call(const char *what, int k, int ret, H264SwDecInst inst)
{
    const h264mi_tensor_desc *t = &g_desc.f.r.t;
    printf("%s %d ret %d calls %d colour %d mode %x layout %d fit %d size %d,%d win %d,%d,%d,%d pad %d,%d,%d nrois %d stride %zu",
           what, k, ret, g_calls, H264SwDecLastTensorColour(inst), t->mode, g_desc.layout, g_desc.f.fit, g_desc.f.r.ow,
           g_desc.f.r.oh, t->x, t->y, t->cw, t->ch, g_desc.f.pad[0], g_desc.f.pad[1], g_desc.f.pad[2], g_nrois, g_stride);
}

/* every descriptor the picture call refuses, one step from a good one; each must come back PARAM_ERR without
 * reaching the engine (and, as the count of delivered pictures shows, without taking a picture) */
static int bad_next(H264SwDecInst inst, int *tried)
{
    int refused = 0;
    const int calls = g_calls;
    H264SwDecPicture pic;
    h264mi_tensor_layout_desc d;
#define BAD(desc, dst)                                                                                              \
    do {                                                                                                            \
        (*tried)++;                                                                                                 \
        refused += H264SwDecNextPictureTensorLayout(inst, &pic, 0, desc, dst, NULL) == H264SWDEC_PARAM_ERR && g_calls == calls; \
    } while (0)
    d = good_desc(0); d.layout = 2; BAD(&d, g_dst);
    d = good_desc(0); d.layout = -1; BAD(&d, g_dst);
    d = good_desc(2); d.layout = 2; BAD(&d, g_dst);
    d = good_desc(0); d.f.fit = H264MI_FIT_LETTERBOX; BAD(&d, g_dst);
    d = good_desc(0); d.f.pad[0] = 1; BAD(&d, g_dst);
    d = good_desc(0); d.f.r.filter = 1; BAD(&d, g_dst);
    d = good_desc(1); d.f.r.oh = 0; BAD(&d, g_dst);
    d = good_desc(1); d.f.r.ow = 0; BAD(&d, g_dst);
    d = good_desc(2); d.f.pad[3] = 1; BAD(&d, g_dst);
    d = good_desc(2); d.f.fit = 3; BAD(&d, g_dst);
    d = good_desc(1); d.f.r.oh = 1; BAD(&d, g_dst);                    /* 52 rows to 1: beyond 32 : 1 */
    d = good_desc(0); d.f.r.t.mode = 2; BAD(&d, g_dst);
    d = good_desc(0); d.f.r.t.mode |= 1 << 14; BAD(&d, g_dst);
    d = good_desc(0); d.f.r.t.dtype = H264MI_TENSOR_I16; BAD(&d, g_dst);
    d = good_desc(0); d.f.r.t.x = 1; d.f.r.t.cw = 4; d.f.r.t.ch = 4; BAD(&d, g_dst);
    d = good_desc(0); BAD(&d, (uint8_t *)g_dst + 1);                    /* fp16 at an odd address */
    d = good_desc(0); BAD(&d, NULL);
    BAD(NULL, g_dst);
#undef BAD
    return refused;
}

static int bad_rois(H264SwDecInst inst, int *tried)
{
    int refused = 0;
    const int calls = g_calls;
    h264mi_tensor_layout_desc d;
    static const h264mi_roi over_right[1] = {{0, 84, 0, 4, 4}}, pic1[1] = {{1, 0, 0, 4, 4}};
#define BAD(desc, rois, n, dst)                                                                                     \
    do {                                                                                                            \
        (*tried)++;                                                                                                 \
        refused += H264SwDecLastPictureTensorRoisLayout(inst, desc, rois, n, dst, NULL) == H264SWDEC_PARAM_ERR &&   \
                   g_calls == calls;                                                                                \
    } while (0)
    d = good_desc(0); BAD(&d, kGood, 2, g_dst);                         /* boxes with no size */
    d = good_desc(1); d.f.r.oh = 0; BAD(&d, kGood, 2, g_dst);
    d = good_desc(1); d.f.r.t.cw = 86; d.f.r.t.ch = 52; BAD(&d, kGood, 2, g_dst);      /* the reserved window */
    d = good_desc(2); d.layout = 2; BAD(&d, kGood, 2, g_dst);
    d = good_desc(2); d.f.pad[3] = 1; BAD(&d, kGood, 2, g_dst);
    d = good_desc(1); BAD(&d, over_right, 1, g_dst);
    d = good_desc(1); BAD(&d, pic1, 1, g_dst);
    d = good_desc(1); BAD(&d, kGood, 0, g_dst);
    d = good_desc(1); BAD(&d, NULL, 2, g_dst);
    d = good_desc(1); BAD(&d, kGood, 2, NULL);
    BAD(NULL, kGood, 2, g_dst);
#undef BAD
    return refused;
}

int main(void)
{
    /* the crop_ltrb_6x4 geometry of tests/golden/crop.json, BT.709 full range in the VUI */
    GenParams p;
    uint8_t *s = NULL;
    size_t n = 0;
    if (h264gen_preset(&p, 2, 61)) return 3;
    p.nframes = 5; p.w_mbs = 6; p.h_mbs = 4; p.slices = 2; p.gop = 3;
    p.crop_left = 6; p.crop_right = 4; p.crop_top = 2; p.crop_bottom = 10;
    p.poc_type = 2;
    p.vui_matrix = 1; p.vui_full_range = 1;
    if (h264gen_generate(&p, &s, &n)) return 3;

    H264SwDecInst inst;
    if (H264SwDecInit(&inst, 0) != H264SWDEC_OK) return 1;
    H264SwDecPicture pic;
    {
        h264mi_tensor_layout_desc d = good_desc(2), bad = good_desc(2);
        bad.layout = 2;
        const int a = H264SwDecNextPictureTensorLayout(inst, &pic, 0, &d, g_dst, NULL);
        const int b = H264SwDecNextPictureTensorFit(inst, &pic, 0, &d.f, g_dst, NULL);
        const int c = H264SwDecLastPictureTensorRoisLayout(inst, &d, kGood, 2, g_dst, NULL);
        const int e = H264SwDecLastPictureTensorRoisFit(inst, &d.f, kGood, 2, g_dst, NULL);
        printf("before next %d mirrored %d rois %d mirrored %d bad_next %d bad_rois %d\n", a, b, c, e,
               H264SwDecNextPictureTensorLayout(inst, &pic, 0, &bad, g_dst, NULL),
               H264SwDecLastPictureTensorRoisLayout(inst, &bad, kGood, 2, g_dst, NULL));
    }
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
            refused += bad_next(inst, &tried);
            const int form = pics % 3;
            h264mi_tensor_layout_desc d = good_desc(form);
            memset(&g_desc, 0xFF, sizeof(g_desc));
            const H264SwDecRet g = H264SwDecNextPictureTensorLayout(inst, &pic, flush, &d, g_dst, NULL);
            if (g != H264SWDEC_PIC_RDY) break;
            flush = 0;
            print_call("pic", pics, g, inst);
            printf("\n");
            refused += bad_rois(inst, &tried);
            d = good_desc(1 + pics % 2);
            memset(&g_desc, 0xFF, sizeof(g_desc));
            const H264SwDecRet b = H264SwDecLastPictureTensorRoisLayout(inst, &d, kGood, 2, g_dst, NULL);
            print_call("box", pics, b, inst);
            printf(" boxes");
            for (int k = 0; k < g_nrois && k < 4; k++)
                printf(" %d,%d,%d,%d,%d", g_rois[k].pic, g_rois[k].x, g_rois[k].y, g_rois[k].cw, g_rois[k].ch);
            printf("\n");
            pics++;
        }
    }
    printf("refused %d of %d then %d\n", refused, tried, pics);
    H264SwDecRelease(inst);
    h264gen_free(s);
    return 0;
}
