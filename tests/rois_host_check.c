/* Host side of H264SwDecLastPictureTensorRois, with no GPU: the
 * product host path (api.c, decoder.c, dpb.c, hipback.cpp) on the CPU stand-in
 * of the engine (oracle/null_device.cpp), which has no export.  The engine
 * export defined here launches nothing and records what it is handed -- or,
 * built with -DNO_EXPORT, is absent, and the backend then has no member for the
 * call.  tests/test_rois_host.py builds both with AddressSanitizer + UBSan, runs
 * them and reads their lines:
 *   before <ret>                         the call before any picture
 *   pic <k> ret <ret> calls <n> colour <id> mode <hex> pics <n> stride <bytes> boxes <pic>,<x>,<y>,<cw>,<ch> ...
 *   refused <bad calls refused without reaching the engine> of <bad calls>
 *   after_decode <ret> ...               the call after each H264SwDecDecode that delivered nothing
 */
#include "../include/h264mi.h"
#include "../broadway_amd/csrc/gen/h264gen.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_calls, g_mode, g_n, g_nrois;
static size_t g_stride;
static h264mi_roi g_rois[4];

#ifndef NO_EXPORT
int h264mi_engine_export_tensor_rois(h264mi_engine *e, int n, const int *streams, const int *slots,
                                     const h264mi_tensor_resize_desc *desc, const h264mi_roi *rois, int nrois,
                                     void *d_out, size_t out_stride, void *hip_stream)
{
    (void)e; (void)streams; (void)slots; (void)d_out; (void)hip_stream;
    g_calls++;
    g_mode = desc->t.mode;
    g_n = n;
    g_nrois = nrois;
    g_stride = out_stride;
    for (int k = 0; k < nrois && k < 4; k++) g_rois[k] = rois[k];
    return desc->t.x | desc->t.y | desc->t.cw | desc->t.ch ? -1 : 0;      /* (the reserved window arrives zero) */
}
#endif

static uint64_t g_dst[4];       /* "device" memory no export writes */

static h264mi_tensor_resize_desc good_desc(void)
{
    h264mi_tensor_resize_desc r;
    memset(&r, 0, sizeof(r));
    r.t.mode = H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_STREAM, H264MI_TENSOR_UNSPEC_BT601);
    r.t.dtype = H264MI_TENSOR_F16;
    r.ow = 9; r.oh = 7; r.filter = H264MI_RESIZE_TRIANGLE;
    return r;
}

/* in the delivered window, 86 x 52: the whole of it, and 4 x 4 flush with its far corner */
static const h264mi_roi kGood[2] = {{0, 0, 0, 86, 52}, {0, 82, 48, 4, 4}};

static H264SwDecRet good_call(H264SwDecInst inst)
{
    const h264mi_tensor_resize_desc r = good_desc();
    return H264SwDecLastPictureTensorRois(inst, &r, kGood, 2, g_dst, NULL);
}

/* every call the export refuses, one step from the good one; returns how many came back PARAM_ERR untouched */
static int bad_calls(H264SwDecInst inst, int *tried)
{
    int refused = 0;
    const int calls = g_calls;
#define BAD(desc, rois, n, dst)                                                                                     \
    do {                                                                                                            \
        (*tried)++;                                                                                                 \
        refused += H264SwDecLastPictureTensorRois(inst, desc, rois, n, dst, NULL) == H264SWDEC_PARAM_ERR && g_calls == calls; \
    } while (0)
    h264mi_tensor_resize_desc r = good_desc();
    static const h264mi_roi over_right[1] = {{0, 84, 0, 4, 4}}, over_bottom[1] = {{0, 0, 50, 4, 4}},
                            pic1[1] = {{1, 0, 0, 4, 4}}, odd_x[1] = {{0, 1, 0, 4, 4}}, negative[1] = {{0, -2, 0, 4, 4}},
                            empty[1] = {{0, 0, 0, 0, 4}}, steep[1] = {{0, 0, 0, 86, 34}},
                            last_bad[3] = {{0, 0, 0, 86, 52}, {0, 82, 48, 4, 4}, {0, 0, 0, 88, 52}};
    BAD(&r, over_right, 1, g_dst);
    BAD(&r, over_bottom, 1, g_dst);
    BAD(&r, pic1, 1, g_dst);
    BAD(&r, odd_x, 1, g_dst);
    BAD(&r, negative, 1, g_dst);
    BAD(&r, empty, 1, g_dst);
    BAD(&r, last_bad, 3, g_dst);
    BAD(&r, kGood, 0, g_dst);
    BAD(&r, NULL, 2, g_dst);
    BAD(NULL, kGood, 2, g_dst);
    BAD(&r, kGood, 2, NULL);
    BAD(&r, kGood, 2, (uint8_t *)g_dst + 1);            /* fp16 at an odd address */
    r.oh = 1;
    BAD(&r, steep, 1, g_dst);                           /* 34 rows to 1: beyond 32 : 1 */
    r = good_desc(); r.t.cw = 86; r.t.ch = 52;
    BAD(&r, kGood, 2, g_dst);                           /* the reserved window */
    r = good_desc(); r.ow = 0;
    BAD(&r, kGood, 2, g_dst);
    r = good_desc(); r.filter = 1;
    BAD(&r, kGood, 2, g_dst);
    r = good_desc(); r.t.dtype = H264MI_TENSOR_I16;
    BAD(&r, kGood, 2, g_dst);
    r = good_desc(); r.t.mode = H264MI_TENSOR_MODE(H264MI_TENSOR_GRAY, H264MI_TENSOR_COLOUR_STREAM, 0);
    BAD(&r, kGood, 2, g_dst);
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
    printf("before %d\n", good_call(inst));
    H264SwDecInput in;
    H264SwDecOutput out;
    H264SwDecPicture pic;
    memset(&in, 0, sizeof(in));
    in.pStream = s;
    in.dataLen = (u32)n;
    int pics = 0, tried = 0, refused = 0;
    char after[1024];
    size_t al = 0;
    after[0] = 0;
    while (in.dataLen > 0) {
        /* one NAL unit per call, as the callers that decode slice by slice feed it */
        u32 len = 4;
        while (len + 3 <= in.dataLen && !(in.pStream[len] == 0 && in.pStream[len + 1] == 0 && in.pStream[len + 2] == 1)) len++;
        if (len + 3 > in.dataLen) len = in.dataLen;
        else if (in.pStream[len - 1] == 0) len--;
        H264SwDecInput one = in;
        one.dataLen = len;
        one.picId = (u32)pics;
        const H264SwDecRet r = H264SwDecDecode(inst, &one, &out);
        in.pStream += len;
        in.dataLen -= len;
        if (r != H264SWDEC_PIC_RDY && r != H264SWDEC_PIC_RDY_BUFF_NOT_EMPTY) {
            if (pics && al + 8 < sizeof(after)) al += (size_t)snprintf(after + al, sizeof(after) - al, " %d", good_call(inst));
            continue;
        }
        while (H264SwDecNextPicture(inst, &pic, 0) == H264SWDEC_PIC_RDY) {
            refused += bad_calls(inst, &tried);
            g_mode = -1;
            const H264SwDecRet g = good_call(inst);
            printf("pic %d ret %d calls %d colour %d mode %x pics %d stride %zu boxes", pics, g, g_calls,
                   H264SwDecLastTensorColour(inst), g_mode, g_n, g_stride);
            for (int k = 0; k < g_nrois && k < 4; k++)
                printf(" %d,%d,%d,%d,%d", g_rois[k].pic, g_rois[k].x, g_rois[k].y, g_rois[k].cw, g_rois[k].ch);
            printf("\n");
            pics++;
        }
    }
    printf("refused %d of %d\n", refused, tried);
    printf("after_decode%s\n", after);
    H264SwDecRelease(inst);
    h264gen_free(s);
    return 0;
}
