/* Host side of H264SwDecLastPictureTensorWarps, with no GPU: the
 * product host path (api.c, decoder.c, dpb.c, hipback.cpp) on the CPU stand-in
 * of the engine (oracle/null_device.cpp), which has no export.  The engine
 * export defined here launches nothing and records what it is handed.
 * tests/test_warp_host.py builds this with AddressSanitizer + UBSan, runs it and
 * reads its lines:
 *   before <ret> bad <ret>               the call before any picture, good and with a bad descriptor
 *   pic <k> form <f> ret <ret> calls <n> colour <id> mode <hex> pics <n> stride <bytes> win <x>,<y>,<cw>,<ch>
 *       size <ow>,<oh> border <b> pad <r>,<g>,<b> layout <l> warps <pic>:<m0>,..,<m5> ...
 *   refused <bad calls refused without reaching the engine> of <bad calls> then <pictures delivered>
 *   after_decode <ret> ...               the call after each H264SwDecDecode that delivered nothing
 * form 0: the window left to the call (cw == 0: the SPS crop window); form 1: a
 * window of its own, (4, 2, 80, 48) in the delivered picture's coordinates. */
#include "../include/h264mi.h"
#include "../broadway_amd/csrc/gen/h264gen.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_calls, g_n, g_nwarps;
static size_t g_stride;
static h264mi_tensor_warp_desc g_desc;
static h264mi_warp g_warps[4];

int h264mi_engine_export_tensor_warps(h264mi_engine *e, int n, const int *streams, const int *slots,
                                      const h264mi_tensor_warp_desc *desc, const h264mi_warp *warps, int nwarps,
                                      void *d_out, size_t out_stride, void *hip_stream)
{
    (void)e; (void)streams; (void)slots; (void)d_out; (void)hip_stream;
    g_calls++;
    g_desc = *desc;
    g_n = n;
    g_nwarps = nwarps;
    g_stride = out_stride;
    for (int k = 0; k < nwarps && k < 4; k++) g_warps[k] = warps[k];
    return 0;
}

static uint64_t g_dst[4];       /* "device" memory no export writes */

static h264mi_tensor_warp_desc good_desc(int form)
{
    h264mi_tensor_warp_desc d;
    memset(&d, 0, sizeof(d));
    d.t.mode = H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_STREAM, H264MI_TENSOR_UNSPEC_BT601);
    d.t.dtype = H264MI_TENSOR_F16;
    d.ow = 9; d.oh = 7; d.filter = H264MI_WARP_BILINEAR;
    if (form) {
        d.t.x = 4; d.t.y = 2; d.t.cw = 80; d.t.ch = 48;
        d.border = H264MI_WARP_BORDER_REPLICATE;
        d.layout = H264MI_LAYOUT_INTERLEAVED;
    } else {
        d.border = H264MI_WARP_BORDER_CONSTANT;
        d.pad[0] = 114; d.pad[1] = 7; d.pad[2] = 250;
    }
    return d;
}

/* the identity, and one with every coefficient extreme: the matrices are the caller's, untouched */
static const h264mi_warp kGood[2] = {{0, {65536, 0, 0, 0, 65536, 0}}, {0, {INT_MIN, INT_MAX, -1, 1, INT_MAX, INT_MIN}}};

static H264SwDecRet good_call(H264SwDecInst inst, int form)
{
    const h264mi_tensor_warp_desc d = good_desc(form);
    return H264SwDecLastPictureTensorWarps(inst, &d, kGood, 2, g_dst, NULL);
}

/* every call the export refuses, one step from a good one; returns how many came back PARAM_ERR untouched */
static int bad_calls(H264SwDecInst inst, int *tried)
{
    int refused = 0;
    const int calls = g_calls;
#define BAD(desc, warps, n, dst)                                                                                    \
    do {                                                                                                            \
        (*tried)++;                                                                                                 \
        refused += H264SwDecLastPictureTensorWarps(inst, desc, warps, n, dst, NULL) == H264SWDEC_PARAM_ERR && g_calls == calls; \
    } while (0)
    h264mi_tensor_warp_desc d = good_desc(0);
    static const h264mi_warp pic1[1] = {{1, {65536, 0, 0, 0, 65536, 0}}},
                             last_bad[2] = {{0, {65536, 0, 0, 0, 65536, 0}}, {-1, {65536, 0, 0, 0, 65536, 0}}};
    BAD(&d, pic1, 1, g_dst);
    BAD(&d, last_bad, 2, g_dst);
    BAD(&d, kGood, 0, g_dst);
    BAD(&d, NULL, 2, g_dst);
    BAD(NULL, kGood, 2, g_dst);
    BAD(&d, kGood, 2, NULL);
    BAD(&d, kGood, 2, (uint8_t *)g_dst + 1);            /* fp16 at an odd address */
    d = good_desc(0); d.ow = 0; BAD(&d, kGood, 2, g_dst);
    d = good_desc(0); d.oh = 16385; BAD(&d, kGood, 2, g_dst);
    d = good_desc(0); d.filter = 1; BAD(&d, kGood, 2, g_dst);
    d = good_desc(0); d.border = 2; BAD(&d, kGood, 2, g_dst);
    d = good_desc(0); d.pad[3] = 1; BAD(&d, kGood, 2, g_dst);
    d = good_desc(0); d.border = H264MI_WARP_BORDER_REPLICATE; BAD(&d, kGood, 2, g_dst);      /* pad with REPLICATE */
    d = good_desc(0); d.layout = 2; BAD(&d, kGood, 2, g_dst);
    d = good_desc(0); d.t.dtype = H264MI_TENSOR_I16; BAD(&d, kGood, 2, g_dst);
    d = good_desc(0); d.t.mode = H264MI_TENSOR_MODE(H264MI_TENSOR_GRAY, H264MI_TENSOR_COLOUR_STREAM, 0); BAD(&d, kGood, 2, g_dst);
    d = good_desc(0); d.t.mode |= 1 << 14; BAD(&d, kGood, 2, g_dst);
    /* the window, in the delivered picture of 86 x 52 */
    d = good_desc(1); d.t.cw = 84; BAD(&d, kGood, 2, g_dst);                                  /* 4 + 84 > 86 */
    d = good_desc(1); d.t.ch = 52; BAD(&d, kGood, 2, g_dst);                                  /* 2 + 52 > 52 */
    d = good_desc(1); d.t.x = 3; BAD(&d, kGood, 2, g_dst);
    d = good_desc(1); d.t.x = -2; BAD(&d, kGood, 2, g_dst);
    d = good_desc(1); d.t.ch = 0; BAD(&d, kGood, 2, g_dst);
    d = good_desc(1); d.t.cw = 79; BAD(&d, kGood, 2, g_dst);
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
        h264mi_tensor_warp_desc bad = good_desc(0);
        bad.border = 2;
        printf("before %d bad %d\n", good_call(inst, 0), H264SwDecLastPictureTensorWarps(inst, &bad, kGood, 2, g_dst, NULL));
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
            const int form = pics & 1;
            memset(&g_desc, 0xFF, sizeof(g_desc));
            const H264SwDecRet g = good_call(inst, form);
            const h264mi_tensor_desc *t = &g_desc.t;
            printf("pic %d form %d ret %d calls %d colour %d mode %x pics %d stride %zu win %d,%d,%d,%d size %d,%d border %d "
                   "pad %d,%d,%d layout %d warps",
                   pics, form, g, g_calls, H264SwDecLastTensorColour(inst), t->mode, g_n, g_stride, t->x, t->y, t->cw, t->ch,
                   g_desc.ow, g_desc.oh, g_desc.border, g_desc.pad[0], g_desc.pad[1], g_desc.pad[2], g_desc.layout);
            for (int k = 0; k < g_nwarps && k < 4; k++)
                printf(" %d:%d,%d,%d,%d,%d,%d", g_warps[k].pic, g_warps[k].m[0], g_warps[k].m[1], g_warps[k].m[2],
                       g_warps[k].m[3], g_warps[k].m[4], g_warps[k].m[5]);
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
