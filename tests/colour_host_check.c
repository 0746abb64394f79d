/* Host side of the tensor colour sets, with no GPU: the
 * generator's VUI writer, parse_vui / H264SwDecGetInfo, the colour pair kept
 * per DPB picture, the resolution of H264MI_TENSOR_COLOUR_STREAM and the
 * checks H264SwDecNextPictureTensor[Resized] make before they take a picture.
 * A stand-alone program: the product host path (api.c, decoder.c, dpb.c,
 * hipback.cpp) on the CPU stand-in of the engine (oracle/null_device.cpp),
 * which has no tensor export -- the two engine exports defined here launch
 * nothing and record the descriptor they are handed.  tests/test_colour.py
 * builds it with AddressSanitizer + UBSan, runs it and reads its lines:
 *   info <matrix> <full> -> <videoRange> <matrixCoefficients>
 *   case <name> pics <n> :  <colour id>/<mode the engine got, hex>/<matrixCoefficients of the
 *                           SPS active at the call, H264SwDecGetInfo> ...
 *   refusals <bad calls refused> of <bad calls> then <pictures delivered>
 *   resolve <rows walked> bad <rows outside 0..3>
 */
#include "../include/h264mi.h"
#include "../broadway_amd/csrc/gen/h264gen.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_mode, g_calls;

int h264mi_engine_export_tensor(h264mi_engine *e, int n, const int *streams, const int *slots,
                                const h264mi_tensor_desc *desc, void *d_out, size_t out_stride, void *hip_stream)
{
    (void)e; (void)n; (void)streams; (void)slots; (void)d_out; (void)out_stride; (void)hip_stream;
    g_mode = desc->mode;
    g_calls++;
    return 0;
}

int h264mi_engine_export_tensor_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                        const h264mi_tensor_resize_desc *desc, void *d_out, size_t out_stride,
                                        void *hip_stream)
{
    (void)e; (void)n; (void)streams; (void)slots; (void)d_out; (void)out_stride; (void)hip_stream;
    g_mode = desc->t.mode;
    g_calls++;
    return 0;
}

typedef struct { uint8_t *p; size_t n; } Buf;

/* the crop_ltrb_6x4 geometry of tests/golden/crop.json with a VUI */
static Buf make_stream(int matrix, int full, int poc_type, unsigned seed)
{
    GenParams p;
    Buf b = {NULL, 0};
    if (h264gen_preset(&p, 2, seed)) exit(3);
    p.nframes = 5; p.w_mbs = 6; p.h_mbs = 4; p.slices = 2; p.gop = 3;
    p.crop_left = 6; p.crop_right = 4; p.crop_top = 2; p.crop_bottom = 10;
    p.poc_type = poc_type;
    p.vui_matrix = matrix; p.vui_full_range = full;
    if (h264gen_generate(&p, &b.p, &b.n)) exit(3);
    return b;
}

static uint64_t g_dst[4];       /* "device" memory no export writes */

/* one tensor call with `mode`; the descriptor takes the SPS crop window */
static H264SwDecRet next_tensor(H264SwDecInst inst, H264SwDecPicture *pic, u32 flush, int mode, int resized)
{
    h264mi_tensor_resize_desc r;
    memset(&r, 0, sizeof(r));
    r.t.mode = mode;
    r.t.dtype = H264MI_TENSOR_U8;
    r.ow = 9; r.oh = 7; r.filter = H264MI_RESIZE_TRIANGLE;
    return resized ? H264SwDecNextPictureTensorResized(inst, pic, flush, &r, g_dst, NULL)
                   : H264SwDecNextPictureTensor(inst, pic, flush, &r.t, g_dst, NULL);
}

static const int kBadModes[] = {
    H264MI_TENSOR_MODE(H264MI_TENSOR_GRAY, H264MI_TENSOR_COLOUR_BT709, 0),
    H264MI_TENSOR_MODE(H264MI_TENSOR_GRAY, H264MI_TENSOR_COLOUR_STREAM, 0),
    H264MI_TENSOR_MODE(H264MI_TENSOR_GRAY, 0, H264MI_TENSOR_UNSPEC_BT709),
    H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, 4, 0), H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, 14, 0),
    H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_STREAM, 3),
    H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_BT709, 0) | 1 << 14,
    H264MI_TENSOR_RGB | 1 << 30, 2, -1,
};
#define NBAD ((int)(sizeof(kBadModes) / sizeof(kBadModes[0])))

/* decode `s`, every picture fetched as a tensor with `mode`; before each
 * fetch (refuse != 0) every bad mode is tried first */
static int decode_case(const char *name, Buf s, int mode, int resized, int refuse)
{
    H264SwDecInst inst;
    if (H264SwDecInit(&inst, 0) != H264SWDEC_OK) return 1;
    if (H264SwDecLastTensorColour(inst) != -1) return 1;
    uint8_t *work = (uint8_t *)malloc(s.n);
    memcpy(work, s.p, s.n);
    H264SwDecInput in;
    H264SwDecOutput out;
    H264SwDecPicture pic;
    memset(&in, 0, sizeof(in));
    in.pStream = work;
    in.dataLen = (u32)s.n;
    int pics = 0, bad = 0, refused = 0, done = 0;
    char line[4096];
    size_t ll = 0;
    line[0] = 0;
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
            if (refuse)
                for (int k = 0; k < NBAD; k++) {
                    const int calls = g_calls;
                    bad++;
                    refused += next_tensor(inst, &pic, 0, kBadModes[k], k & 1) == H264SWDEC_PARAM_ERR && g_calls == calls;
                }
            g_mode = -1;
            if (next_tensor(inst, &pic, flush, mode, resized) != H264SWDEC_PIC_RDY) break;
            flush = 0;
            pics++;
            H264SwDecInfo info;
            if (H264SwDecGetInfo(inst, &info) != H264SWDEC_OK) info.matrixCoefficients = 999;
            if (ll + 48 < sizeof(line))
                ll += (size_t)snprintf(line + ll, sizeof(line) - ll, " %d/%x/%u", H264SwDecLastTensorColour(inst), g_mode,
                                       info.matrixCoefficients);
        }
    }
    printf("case %s pics %d :%s\n", name, pics, line);
    if (refuse) printf("refusals %d of %d then %d\n", refused, bad, pics);
    H264SwDecRelease(inst);
    free(work);
    return 0;
}

static int info_line(int matrix, int full)
{
    Buf s = make_stream(matrix, full, 2, 61);
    H264SwDecInst inst;
    if (H264SwDecInit(&inst, 0) != H264SWDEC_OK) return 1;
    H264SwDecInput in;
    H264SwDecOutput out;
    H264SwDecInfo info;
    memset(&in, 0, sizeof(in));
    in.pStream = s.p;
    in.dataLen = (u32)s.n;
    int rc = 1;
    while (in.dataLen > 0) {
        const H264SwDecRet r = H264SwDecDecode(inst, &in, &out);
        if (r == H264SWDEC_HDRS_RDY_BUFF_NOT_EMPTY) {
            if (H264SwDecGetInfo(inst, &info) == H264SWDEC_OK) {
                printf("info %d %d -> %u %u\n", matrix, full, info.videoRange, info.matrixCoefficients);
                rc = 0;
            }
            break;
        }
        const u32 used = (u32)(out.pStrmCurrPos - in.pStream);
        if (used == 0) break;
        in.dataLen -= used;
        in.pStream = out.pStrmCurrPos;
    }
    H264SwDecRelease(inst);
    h264gen_free(s.p);
    return rc;
}

int main(void)
{
    int rc = 0;
    static const int kMatrix[] = {0, -1, 1, 2, 5, 6, 7};
    for (int m = 0; m < 7; m++)
        for (int full = 0; full < 2; full++) rc |= info_line(kMatrix[m], full);

    const int stream709 = H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_STREAM, H264MI_TENSOR_UNSPEC_BT709);
    const int stream_size = H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_STREAM, H264MI_TENSOR_UNSPEC_SIZE);
    struct { const char *name; int matrix, full, mode, resized; } cases[] = {
        {"m1", 1, 0, stream709, 0}, {"m1_full", 1, 1, stream709, 0}, {"m6_full", 6, 1, stream709, 1},
        {"m7_full", 7, 1, stream709, 0}, {"novui_size", 0, 0, stream_size, 0}, {"sig_full_size", -1, 1, stream_size, 1},
        {"explicit_bt709", 6, 1, H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_BT709, 0), 0},
        {"gray", 1, 1, H264MI_TENSOR_GRAY, 0},
    };
    for (size_t k = 0; k < sizeof(cases) / sizeof(cases[0]); k++) {
        Buf s = make_stream(cases[k].matrix, cases[k].full, 2, 61);
        rc |= decode_case(cases[k].name, s, cases[k].mode, cases[k].resized, k == 0);
        h264gen_free(s.p);
    }

    /* two SPSs with id 0 in one stream: (matrix 1) with display reordering --
     * its last pictures leave the DPB when the second SPS is already active --
     * then (matrix 6, full range) */
    Buf a = make_stream(1, 0, 0, 61), b = make_stream(6, 1, 2, 62), ab;
    ab.n = a.n + b.n;
    ab.p = (uint8_t *)malloc(ab.n);
    memcpy(ab.p, a.p, a.n);
    memcpy(ab.p + a.n, b.p, b.n);
    rc |= decode_case("two_sps", ab, H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_STREAM, 0), 0, 0);
    free(ab.p);
    h264gen_free(a.p);
    h264gen_free(b.p);

    /* the resolution table, every row */
    int rows = 0, bad = 0;
    for (int unspec = 0; unspec < 3; unspec++)
        for (int matrix = 0; matrix < 256; matrix++)
            for (int full = 0; full < 2; full++)
                for (int big = 0; big < 4; big++) {
                    const int cw = big == 1 ? 1280 : 1278, ch = big == 2 ? 578 : 576;
                    const int id = h264mi_tensor_colour_resolve(
                        H264MI_TENSOR_MODE(H264MI_TENSOR_RGB, H264MI_TENSOR_COLOUR_STREAM, unspec), matrix, full, cw, ch);
                    rows++;
                    bad += id < 0 || id > 3 || (id & 1) != full;
                }
    for (int k = 0; k < NBAD; k++) {
        rows++;
        bad += h264mi_tensor_colour_resolve(kBadModes[k], 1, 0, 64, 64) != -1;
    }
    printf("resolve %d bad %d\n", rows, bad);
    return rc || bad;
}
