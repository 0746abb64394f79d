/* The descriptor rules of the accumulated-residual export
 * (broadway_amd/csrc/common/export_desc.h) walked over a small grid on a 6 x 4
 * MB picture (96 x 64 luma samples), as tests/accmv_desc_check.c walks its
 * own: one line per row, "accres <row> accept|refuse", a descriptor being
 * accepted when both of its parts pass.  tests/test_accres.py holds the
 * expected column.  Built with AddressSanitizer + UBSan. */
#include <stdio.h>
#include <string.h>

#include "../broadway_amd/csrc/common/export_desc.h"

enum { W_MBS = 6, H_MBS = 4 };

static void accres_on(const char *name, int w_mbs, int h_mbs, int x, int y, int cw, int ch, int planes, int dtype,
                      int colour, int unanchored)
{
    h264mi_accres_desc d;
    memset(&d, 0, sizeof(d));
    d.x = x; d.y = y; d.cw = cw; d.ch = ch; d.planes = planes; d.dtype = dtype; d.colour = colour;
    d.unanchored = unanchored;
    printf("accres %s %s\n", name, accres_desc_fixed_ok(&d) && accres_window_ok(&d, w_mbs, h_mbs) ? "accept" : "refuse");
}

static void accres(const char *name, int x, int y, int cw, int ch, int planes, int dtype, int colour, int unanchored)
{
    accres_on(name, W_MBS, H_MBS, x, y, cw, ch, planes, dtype, colour, unanchored);
}

int main(void)
{
    const int U8 = H264MI_TENSOR_U8, F16 = H264MI_TENSOR_F16, BF16 = H264MI_TENSOR_BF16, F32 = H264MI_TENSOR_F32,
              I16 = H264MI_TENSOR_I16;
    const int Y = H264MI_ACCRES_Y, UV = H264MI_ACCRES_UV, YUV = H264MI_ACCRES_YUV, RGB = H264MI_ACCRES_RGB;

    accres("whole", 0, 0, 96, 64, Y, I16, 0, 0);
    accres("flush_right_bottom", 11, 21, 85, 43, Y, I16, 0, 0);
    accres("right_plus_1", 11, 21, 86, 43, Y, I16, 0, 0);
    accres("right_plus_1_by_origin", 12, 21, 85, 43, Y, I16, 0, 0);
    accres("bottom_plus_1", 11, 21, 85, 44, Y, I16, 0, 0);
    accres("bottom_plus_1_by_origin", 11, 22, 85, 43, Y, I16, 0, 0);
    accres("origin_0", 0, 0, 1, 1, Y, I16, 0, 0);
    accres("odd_window_yuv", 3, 5, 7, 9, YUV, I16, 0, 0);
    accres("odd_window_rgb", 3, 5, 7, 9, RGB, I16, 0, 0);
    accres("last_sample", 95, 63, 1, 1, Y, I16, 0, 0);
    accres("x_negative", -1, 0, 4, 4, Y, I16, 0, 0);
    accres("y_negative", 0, -1, 4, 4, Y, I16, 0, 0);
    accres("cw_0", 0, 0, 0, 4, Y, I16, 0, 0);
    accres("ch_0", 0, 0, 4, 0, Y, I16, 0, 0);
    accres("cw_negative", 4, 0, -4, 4, Y, I16, 0, 0);
    accres("ch_negative", 0, 4, 4, -4, Y, I16, 0, 0);
    accres("uv_even", 2, 4, 6, 8, UV, I16, 0, 0);
    accres("uv_whole", 0, 0, 96, 64, UV, I16, 0, 0);
    accres("uv_odd_x", 1, 4, 6, 8, UV, I16, 0, 0);
    accres("uv_odd_y", 2, 3, 6, 8, UV, I16, 0, 0);
    accres("uv_odd_cw", 2, 4, 5, 8, UV, I16, 0, 0);
    accres("uv_odd_ch", 2, 4, 6, 7, UV, I16, 0, 0);
    accres("dtype_u8", 0, 0, 4, 4, Y, U8, 0, 0);
    accres("dtype_f16", 0, 0, 4, 4, Y, F16, 0, 0);
    accres("dtype_bf16", 0, 0, 4, 4, Y, BF16, 0, 0);
    accres("dtype_f32", 0, 0, 4, 4, Y, F32, 0, 0);
    accres("dtype_5", 0, 0, 4, 4, Y, 5, 0, 0);
    accres("dtype_minus_1", 0, 0, 4, 4, Y, -1, 0, 0);
    accres("planes_rgb", 0, 0, 4, 4, RGB, I16, 0, 0);
    accres("planes_4", 0, 0, 4, 4, 4, I16, 0, 0);
    accres("planes_minus_1", 0, 0, 4, 4, -1, I16, 0, 0);
    accres("colour_3", 0, 0, 4, 4, RGB, I16, 3, 0);
    accres("colour_4", 0, 0, 4, 4, RGB, I16, 4, 0);
    accres("colour_stream", 0, 0, 4, 4, RGB, I16, H264MI_TENSOR_COLOUR_STREAM, 0);
    accres("colour_stream_y", 0, 0, 4, 4, Y, I16, H264MI_TENSOR_COLOUR_STREAM, 0);
    accres("colour_minus_1", 0, 0, 4, 4, RGB, I16, -1, 0);
    accres("policy_zero", 0, 0, 4, 4, Y, I16, 0, H264MI_ACCRES_ZERO);
    accres("policy_2", 0, 0, 4, 4, Y, I16, 0, 2);
    accres("policy_minus_1", 0, 0, 4, 4, Y, I16, 0, -1);
    /* the origin maps it reads hold 15-bit coordinates: 2048 MBs each way */
    accres_on("wide_2048_mbs", 2048, 1, 32767, 15, 1, 1, Y, I16, 0, 0);
    accres_on("wide_2049_mbs", 2049, 1, 0, 0, 1, 1, Y, I16, 0, 0);
    accres_on("tall_2048_mbs", 1, 2048, 15, 32767, 1, 1, Y, I16, 0, 0);
    accres_on("tall_2049_mbs", 1, 2049, 0, 0, 1, 1, Y, I16, 0, 0);
    return 0;
}
