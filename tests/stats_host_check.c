/* Host side of H264SwDecLastPictureStats, with no GPU: the
 * product host path (api.c, decoder.c, dpb.c, hipback.cpp) on the CPU stand-in
 * of the engine (oracle/null_device.cpp), which has no export.  The engine
 * export defined here launches nothing and records what it is handed.
 * tests/test_stats_host.py builds this with AddressSanitizer + UBSan, runs it
 * and reads its lines:
 *   before <ret> bad <ret>               the call before any picture, good and with a bad descriptor
 *   pic <k> form <f> ret <ret> calls <n> colour <id> planes <p> dcolour <id> flags <f> reserved <r> pics <n> ref <0|1>
 *       stride <bytes> win <x>,<y>,<cw>,<ch> boxes <pic>:<x>,<y>,<cw>,<ch> ...
 *   refused <bad calls refused without reaching the engine> of <bad calls> then <pictures delivered>
 *   after_decode <ret> ...               the call after each H264SwDecDecode that delivered nothing
 * form 0: RGB with the histogram and the stream's colour, the window left to
 * the call (cw == 0: the SPS crop window); form 1: YUV, a window of its own,
 * (4, 2, 80, 48) in the delivered picture's coordinates; form 2: Y with the
 * histogram over three boxes. */
#include "../include/h264mi.h"
#include "../broadway_amd/csrc/gen/h264gen.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_calls, g_n, g_nrois, g_ref;
static size_t g_stride;
static h264mi_stats_desc g_desc;
static h264mi_roi g_rois[4];

int h264mi_engine_export_stats(h264mi_engine *e, int n, const int *streams, const int *slots, const int *ref_streams,
                               const int *ref_slots, const h264mi_stats_desc *desc, const h264mi_roi *rois, int nrois,
                               void *d_out, size_t out_stride, void *hip_stream)
{
    (void)e; (void)streams; (void)slots; (void)d_out; (void)hip_stream;
    g_calls++;
    g_desc = *desc;
    g_n = n;
    g_ref = ref_streams != NULL || ref_slots != NULL;
    g_nrois = nrois;
    g_stride = out_stride;
    for (int k = 0; rois && k < nrois && k < 4; k++) g_rois[k] = rois[k];
    return 0;
}

static uint64_t g_dst[4];       /* "device" memory no export writes */

static h264mi_stats_desc good_desc(int form)
{
    h264mi_stats_desc d;
    memset(&d, 0, sizeof(d));
    if (form == 0) {
        d.planes = H264MI_STATS_RGB; d.colour = H264MI_TENSOR_COLOUR_STREAM; d.flags = H264MI_STATS_HIST;
    } else if (form == 1) {
        d.planes = H264MI_STATS_YUV;
        d.x = 4; d.y = 2; d.cw = 80; d.ch = 48;
    } else {
        d.planes = H264MI_STATS_Y; d.flags = H264MI_STATS_HIST;
    }
    return d;
}

/* in the delivered picture of 86 x 52: all of it, a box at its right and bottom edges, a 2 x 2 box */
static const h264mi_roi kBoxes[3] = {{0, 0, 0, 86, 52}, {0, 46, 20, 40, 32}, {0, 2, 2, 2, 2}};

static H264SwDecRet good_call(H264SwDecInst inst, int form)
{
    const h264mi_stats_desc d = good_desc(form);
    return H264SwDecLastPictureStats(inst, &d, form == 2 ? kBoxes : NULL, form == 2 ? 3 : 0, g_dst, NULL);
}

/* every call the export refuses, one step from a good one; returns how many came back PARAM_ERR untouched */
static int bad_calls(H264SwDecInst inst, int *tried)
{
    int refused = 0;
    const int calls = g_calls;
#define BAD(desc, rois, n, dst)                                                                                      \
    do {                                                                                                             \
        (*tried)++;                                                                                                  \
        refused += H264SwDecLastPictureStats(inst, desc, rois, n, dst, NULL) == H264SWDEC_PARAM_ERR && g_calls == calls; \
    } while (0)
    h264mi_stats_desc d = good_desc(0);
    BAD(NULL, NULL, 0, g_dst);
    BAD(&d, NULL, 0, NULL);
    BAD(&d, NULL, 0, (uint8_t *)g_dst + 4);              /* int64 words at an address that is no multiple of 8 */
    BAD(&d, NULL, 1, g_dst);                             /* a count without boxes */
    d = good_desc(0); d.planes = 3; BAD(&d, NULL, 0, g_dst);
    d = good_desc(0); d.planes = -1; BAD(&d, NULL, 0, g_dst);
    d = good_desc(0); d.flags = 2; BAD(&d, NULL, 0, g_dst);
    d = good_desc(0); d.flags = 3; BAD(&d, NULL, 0, g_dst);
    d = good_desc(0); d.reserved = 1; BAD(&d, NULL, 0, g_dst);
    d = good_desc(0); d.colour = 4; BAD(&d, NULL, 0, g_dst);
    d = good_desc(0); d.colour = -1; BAD(&d, NULL, 0, g_dst);
    d = good_desc(1); d.colour = 1; BAD(&d, NULL, 0, g_dst);                                    /* a colour with YUV */
    d = good_desc(2); d.colour = H264MI_TENSOR_COLOUR_STREAM; BAD(&d, kBoxes, 3, g_dst);          /* STREAM with Y */
    /* the window, in the delivered picture of 86 x 52 */
    d = good_desc(1); d.cw = 84; BAD(&d, NULL, 0, g_dst);                                        /* 4 + 84 > 86 */
    d = good_desc(1); d.ch = 52; BAD(&d, NULL, 0, g_dst);                                        /* 2 + 52 > 52 */
    d = good_desc(1); d.x = 3; BAD(&d, NULL, 0, g_dst);
    d = good_desc(1); d.x = -2; BAD(&d, NULL, 0, g_dst);
    d = good_desc(1); d.x = INT_MAX - 1; BAD(&d, NULL, 0, g_dst);
    d = good_desc(1); d.ch = 0; BAD(&d, NULL, 0, g_dst);
    d = good_desc(1); d.cw = 79; BAD(&d, NULL, 0, g_dst);
    d = good_desc(1); d.cw = 0; BAD(&d, NULL, 0, g_dst);                                         /* cw == 0 with the rest set */
    /* boxes */
    d = good_desc(2);
    BAD(&d, kBoxes, 0, g_dst);
    d = good_desc(2); d.cw = 2; d.ch = 2; BAD(&d, kBoxes, 3, g_dst);                             /* a window with boxes */
    d = good_desc(2);
    h264mi_roi b[3];
    memcpy(b, kBoxes, sizeof(b)); b[2].pic = 1; BAD(&d, b, 3, g_dst);
    memcpy(b, kBoxes, sizeof(b)); b[1].cw = 42; BAD(&d, b, 3, g_dst);                            /* 46 + 42 > 86 */
    memcpy(b, kBoxes, sizeof(b)); b[1].ch = 34; BAD(&d, b, 3, g_dst);                            /* 20 + 34 > 52 */
    memcpy(b, kBoxes, sizeof(b)); b[2].x = 3; BAD(&d, b, 3, g_dst);
    memcpy(b, kBoxes, sizeof(b)); b[0].x = -2; BAD(&d, b, 3, g_dst);
    memcpy(b, kBoxes, sizeof(b)); b[2].ch = 0; BAD(&d, b, 3, g_dst);
    memcpy(b, kBoxes, sizeof(b)); b[0].y = INT_MAX - 1; BAD(&d, b, 3, g_dst);
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
    {
        h264mi_stats_desc bad = good_desc(0);
        bad.flags = 2;
        printf("before %d bad %d\n", good_call(inst, 0), H264SwDecLastPictureStats(inst, &bad, NULL, 0, g_dst, NULL));
    }
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
            if (pics && al + 8 < sizeof(after)) al += (size_t)snprintf(after + al, sizeof(after) - al, " %d", good_call(inst, 0));
            continue;
        }
        while (H264SwDecNextPicture(inst, &pic, 0) == H264SWDEC_PIC_RDY) {
            refused += bad_calls(inst, &tried);
            const int form = pics % 3;
            memset(&g_desc, 0xFF, sizeof(g_desc));
            memset(g_rois, 0xFF, sizeof(g_rois));
            const H264SwDecRet g = good_call(inst, form);
            printf("pic %d form %d ret %d calls %d colour %d planes %d dcolour %d flags %d reserved %d pics %d ref %d stride %zu "
                   "win %d,%d,%d,%d boxes",
                   pics, form, g, g_calls, H264SwDecLastTensorColour(inst), g_desc.planes, g_desc.colour, g_desc.flags,
                   g_desc.reserved, g_n, g_ref, g_stride, g_desc.x, g_desc.y, g_desc.cw, g_desc.ch);
            for (int k = 0; k < g_nrois && k < 4; k++)
                printf(" %d:%d,%d,%d,%d", g_rois[k].pic, g_rois[k].x, g_rois[k].y, g_rois[k].cw, g_rois[k].ch);
            printf("\n");
            pics++;
        }
    }
    printf("refused %d of %d then %d\n", refused, tried, pics);
    printf("after_decode%s\n", after);
    H264SwDecRelease(inst);
    h264gen_free(s);
    return 0;
}
