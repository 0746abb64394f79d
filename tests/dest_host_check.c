/* Host side of H264SwDecNextPictureTensorDest, with no GPU: the
 * product host path (api.c, decoder.c, dpb.c, hipback.cpp) on the CPU stand-in
 * of the engine (oracle/null_device.cpp), which has no export.  The engine
 * export defined here launches nothing and records what it is handed.  Built
 * with -DNO_DEST_EXPORT the program defines no such export, so that the
 * backend has no export_tensor_dest member.  tests/test_dest_host.py builds
 * both with AddressSanitizer + UBSan, runs them and reads their lines:
 *   before dest <ret> bad <ret>
 *   pic <k> ret <ret> calls <n> layout <l> size <ow>,<oh> win <x>,<y>,<cw>,<ch> dest <row>,<plane>,<frame>,<clip>,<reserved>
 *       null <0|1> dst <offset of d_dst in the buffer> nrois <n> stride <bytes> n <pictures>
 *   refused <bad calls refused without reaching the engine> of <bad calls>
 *   plain <pictures H264SwDecNextPicture delivered after a refusal> dest <pictures the dest call delivered>
 *   missing <ret of the dest call> calls <n> plain <pictures delivered>           (NO_DEST_EXPORT)
 */
#include "../include/h264mi.h"
#include "../broadway_amd/csrc/gen/h264gen.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int g_calls, g_nrois, g_n, g_null;
static size_t g_stride;
static void *g_out;
static h264mi_tensor_layout_desc g_desc;
static h264mi_tensor_dest g_dest;

#ifndef NO_DEST_EXPORT
int h264mi_engine_export_tensor_dest(h264mi_engine *e, int n, const int *streams, const int *slots,
                                     const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois, int nrois,
                                     const h264mi_tensor_dest *dest, void *d_out, size_t out_stride, void *hip_stream)
{
    (void)e; (void)streams; (void)slots; (void)rois; (void)hip_stream;
    g_calls++;
    g_desc = *desc;
    g_null = dest == NULL;
    memset(&g_dest, 0xFF, sizeof(g_dest));
    if (dest) g_dest = *dest;
    g_n = n;
    g_nrois = nrois;
    g_stride = out_stride;
    g_out = d_out;
    return 0;
}
#endif

static uint64_t g_dst[8];       /* "device" memory no export writes */

/* form 0: unresized, planar; 1: stretched into 9 x 7, interleaved.  The window is left to the call (cw == 0) */
static h264mi_tensor_layout_desc good_desc(int form)
{
    h264mi_tensor_layout_desc d;
    memset(&d, 0, sizeof(d));
    d.f.r.t.mode = H264MI_TENSOR_RGB;
    d.f.r.t.dtype = H264MI_TENSOR_F16;
    d.layout = form ? H264MI_LAYOUT_INTERLEAVED : H264MI_LAYOUT_PLANAR;
    if (form) { d.f.r.ow = 9; d.f.r.oh = 7; d.f.r.filter = H264MI_RESIZE_TRIANGLE; }
    return d;
}

/* a destination the form's items fit: the delivered window is 86 x 52 fp16 (a packed row 172 bytes), the
 * stretched interleaved item 7 rows of 9 * 3 * 2 = 54 bytes */
static h264mi_tensor_dest good_dest(int form)
{
    h264mi_tensor_dest t;
    memset(&t, 0, sizeof(t));
    t.clip = 1;
    if (form) t.row = 64;
    else { t.row = 176; t.plane = 53 * 176; }
    return t;
}

/* every destination the call refuses, one step from a good one; each must come back PARAM_ERR without reaching
 * the engine and without taking a picture */
static int bad_next(H264SwDecInst inst, int *tried)
{
    int refused = 0;
    const int calls = g_calls;
    H264SwDecPicture pic;
    h264mi_tensor_layout_desc d;
    h264mi_tensor_dest t;
#define BAD(desc, dest, dst)                                                                                        \
    do {                                                                                                            \
        (*tried)++;                                                                                                 \
        refused += H264SwDecNextPictureTensorDest(inst, &pic, 0, desc, dest, dst, NULL) == H264SWDEC_PARAM_ERR &&   \
                   g_calls == calls;                                                                                \
    } while (0)
    d = good_desc(0); t = good_dest(0); t.clip = 2; t.frame = 3 * 53 * 176; BAD(&d, &t, g_dst);   /* one picture is one item */
    d = good_desc(0); t = good_dest(0); t.clip = 0; BAD(&d, &t, g_dst);
    d = good_desc(0); t = good_dest(0); t.frame = 2; BAD(&d, &t, g_dst);
    d = good_desc(0); t = good_dest(0); t.reserved = 1; BAD(&d, &t, g_dst);
    d = good_desc(0); t = good_dest(0); t.row = 170; BAD(&d, &t, g_dst);               /* 86 columns are 172 bytes */
    d = good_desc(0); t = good_dest(0); t.row = 177; BAD(&d, &t, g_dst);
    d = good_desc(0); t = good_dest(0); t.plane = 52 * 176 - 6; BAD(&d, &t, g_dst);    /* into the last row */
    d = good_desc(0); t = good_dest(0); t.row = -176; BAD(&d, &t, g_dst);
    d = good_desc(1); t = good_dest(1); t.plane = 7 * 64; BAD(&d, &t, g_dst);           /* interleaved has no plane */
    d = good_desc(1); t = good_dest(1); t.row = 52; BAD(&d, &t, g_dst);
    d = good_desc(0); d.layout = 2; t = good_dest(0); BAD(&d, &t, g_dst);
    d = good_desc(0); t = good_dest(0); BAD(&d, &t, (uint8_t *)g_dst + 1);              /* fp16 at an odd address */
    d = good_desc(0); t = good_dest(0); BAD(&d, &t, NULL);
    t = good_dest(0); BAD(NULL, &t, g_dst);
#undef BAD
    return refused;
}

int main(void)
{
    /* the crop_ltrb_6x4 geometry of tests/golden/crop.json */
    GenParams p;
    uint8_t *s = NULL;
    size_t n = 0;
    if (h264gen_preset(&p, 2, 61)) return 3;
    p.nframes = 6; p.w_mbs = 6; p.h_mbs = 4; p.slices = 2; p.gop = 3;
    p.crop_left = 6; p.crop_right = 4; p.crop_top = 2; p.crop_bottom = 10;
    p.poc_type = 2;
    if (h264gen_generate(&p, &s, &n)) return 3;

    H264SwDecInst inst;
    if (H264SwDecInit(&inst, 0) != H264SWDEC_OK) return 1;
    H264SwDecPicture pic;
#ifndef NO_DEST_EXPORT
    {
        h264mi_tensor_layout_desc d = good_desc(0);
        h264mi_tensor_dest t = good_dest(0), bad = good_dest(0);
        bad.clip = 2;
        const int a = H264SwDecNextPictureTensorDest(inst, &pic, 0, &d, &t, g_dst, NULL);
        printf("before dest %d bad %d\n", a, H264SwDecNextPictureTensorDest(inst, &pic, 0, &d, &bad, g_dst, NULL));
    }
#endif
    H264SwDecInput in;
    H264SwDecOutput out;
    memset(&in, 0, sizeof(in));
    in.pStream = s;
    in.dataLen = (u32)n;
    int pics = 0, plain = 0, tried = 0, refused = 0, done = 0, missing = 0;
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
#ifdef NO_DEST_EXPORT
            /* no member: PARAM_ERR, and the picture is still there for the plain call */
            h264mi_tensor_layout_desc d = good_desc(0);
            h264mi_tensor_dest t = good_dest(0);
            missing = H264SwDecNextPictureTensorDest(inst, &pic, 0, &d, &t, g_dst, NULL);
            if (H264SwDecNextPicture(inst, &pic, flush) != H264SWDEC_PIC_RDY) break;
            flush = 0;
            plain++;
#else
            refused += bad_next(inst, &tried);
            /* every third picture is taken by the plain call, right after the refusals: they left it in the DPB */
            if ((pics + plain) % 3 == 2) {
                if (H264SwDecNextPicture(inst, &pic, flush) != H264SWDEC_PIC_RDY) break;
                flush = 0;
                plain++;
                continue;
            }
            const int form = pics % 2, null = pics % 4 == 3;
            h264mi_tensor_layout_desc d = good_desc(form);
            h264mi_tensor_dest t = good_dest(form);
            void *dst = (uint8_t *)g_dst + 2 * (pics % 4);
            memset(&g_desc, 0xFF, sizeof(g_desc));
            const H264SwDecRet g = H264SwDecNextPictureTensorDest(inst, &pic, flush, &d, null ? NULL : &t, dst, NULL);
            if (g != H264SWDEC_PIC_RDY) break;
            flush = 0;
            printf("pic %d ret %d calls %d layout %d size %d,%d win %d,%d,%d,%d dest %lld,%lld,%lld,%d,%d null %d dst %td "
                   "nrois %d stride %zu n %d\n", pics, g, g_calls, g_desc.layout, g_desc.f.r.ow, g_desc.f.r.oh,
                   g_desc.f.r.t.x, g_desc.f.r.t.y, g_desc.f.r.t.cw, g_desc.f.r.t.ch, (long long)g_dest.row,
                   (long long)g_dest.plane, (long long)g_dest.frame, g_dest.clip, g_dest.reserved, g_null,
                   (uint8_t *)g_out - (uint8_t *)g_dst, g_nrois, g_stride, g_n);
            pics++;
#endif
        }
    }
#ifdef NO_DEST_EXPORT
    printf("missing %d calls %d plain %d\n", missing, g_calls, plain);
    (void)pics; (void)tried; (void)refused;
#else
    printf("refused %d of %d\n", refused, tried);
    printf("plain %d dest %d\n", plain, pics);
    (void)missing;
#endif
    H264SwDecRelease(inst);
    h264gen_free(s);
    return 0;
}
