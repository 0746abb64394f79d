/* The descriptor rules of the accumulated-motion export
 * (broadway_amd/csrc/common/export_desc.h) walked over a small grid on a 6 x 4
 * MB picture (96 x 64 luma samples), as tests/export_desc_check.c walks the
 * others: one line per row, "accmv <row> accept|refuse", a descriptor being
 * accepted when both of its parts pass; then the picture sizes an origin map
 * can hold.  tests/test_accmv.py holds the expected column.  Built with
 * AddressSanitizer + UBSan. */
#include <stdio.h>
#include <string.h>

#include "../broadway_amd/csrc/common/export_desc.h"

enum { W_MBS = 6, H_MBS = 4 };

static void row(const char *kind, const char *name, int ok) { printf("%s %s %s\n", kind, name, ok ? "accept" : "refuse"); }

static void accmv_on(const char *name, int w_mbs, int h_mbs, int x, int y, int cw, int ch, int dtype, int nch, int last_id)
{
    h264mi_accmv_desc d;
    memset(&d, 0, sizeof(d));
    d.x = x; d.y = y; d.cw = cw; d.ch = ch; d.dtype = dtype; d.nch = nch;
    if (nch >= 1 && nch <= H264MI_ACCMV_MAX_CH) d.id[nch - 1] = last_id;
    row("accmv", name, accmv_desc_fixed_ok(&d) && accmv_window_ok(&d, w_mbs, h_mbs));
}

static void accmv(const char *name, int x, int y, int cw, int ch, int dtype, int nch, int last_id)
{
    accmv_on(name, W_MBS, H_MBS, x, y, cw, ch, dtype, nch, last_id);
}

int main(void)
{
    const int U8 = H264MI_TENSOR_U8, F16 = H264MI_TENSOR_F16, BF16 = H264MI_TENSOR_BF16, F32 = H264MI_TENSOR_F32,
              I16 = H264MI_TENSOR_I16;

    accmv("whole", 0, 0, 96, 64, I16, 2, 1);
    accmv("flush_right_bottom", 11, 21, 85, 43, I16, 2, 1);
    accmv("right_plus_1", 11, 21, 86, 43, I16, 2, 1);
    accmv("right_plus_1_by_origin", 12, 21, 85, 43, I16, 2, 1);
    accmv("bottom_plus_1", 11, 21, 85, 44, I16, 2, 1);
    accmv("bottom_plus_1_by_origin", 11, 22, 85, 43, I16, 2, 1);
    accmv("origin_0", 0, 0, 1, 1, I16, 2, 1);
    accmv("odd_window", 3, 5, 7, 9, I16, 2, 1);
    accmv("last_sample", 95, 63, 1, 1, I16, 2, 1);
    accmv("x_negative", -1, 0, 4, 4, I16, 2, 1);
    accmv("y_negative", 0, -1, 4, 4, I16, 2, 1);
    accmv("cw_0", 0, 0, 0, 4, I16, 2, 1);
    accmv("ch_0", 0, 0, 4, 0, I16, 2, 1);
    accmv("cw_negative", 4, 0, -4, 4, I16, 2, 1);
    accmv("ch_negative", 0, 4, 4, -4, I16, 2, 1);
    accmv("dtype_u8", 0, 0, 4, 4, U8, 2, 1);
    accmv("dtype_f16", 0, 0, 4, 4, F16, 2, 1);
    accmv("dtype_bf16", 0, 0, 4, 4, BF16, 2, 1);
    accmv("dtype_f32", 0, 0, 4, 4, F32, 2, 1);
    accmv("dtype_5", 0, 0, 4, 4, 5, 2, 1);
    accmv("dtype_minus_1", 0, 0, 4, 4, -1, 2, 1);
    accmv("nch_0", 0, 0, 4, 4, I16, 0, 0);
    accmv("nch_1", 0, 0, 4, 4, I16, 1, 0);
    accmv("nch_8", 0, 0, 4, 4, I16, 8, 0);
    accmv("nch_9", 0, 0, 4, 4, I16, 9, 0);
    accmv("nch_negative", 0, 0, 4, 4, I16, -1, 0);
    accmv("channel_minus_1", 0, 0, 4, 4, I16, 2, -1);
    accmv("channel_4", 0, 0, 4, 4, I16, 2, 4);
    accmv("channel_5", 0, 0, 4, 4, I16, 2, 5);
    accmv("channel_5_at_8", 0, 0, 4, 4, I16, 8, 5);
    /* an origin map holds 15-bit coordinates: 2048 MBs each way */
    accmv_on("wide_2048_mbs", 2048, 1, 32767, 15, 1, 1, I16, 1, 0);
    accmv_on("wide_2049_mbs", 2049, 1, 0, 0, 1, 1, I16, 1, 0);
    accmv_on("tall_2048_mbs", 1, 2048, 15, 32767, 1, 1, I16, 1, 0);
    accmv_on("tall_2049_mbs", 1, 2049, 0, 0, 1, 1, I16, 1, 0);
    printf("size %d %d %d %d %d\n", accmv_size_ok(2048, 2048), accmv_size_ok(2049, 1), accmv_size_ok(1, 2049),
           accmv_size_ok(0, 1), accmv_size_ok(1, 0));
    return 0;
}
