/* The descriptor rules of the resized accumulated-motion and accumulated-
 * residual exports (broadway_amd/csrc/common/export_desc.h) walked over a small
 * grid, as tests/accmv_desc_check.c walks the unresized ones: one line per row,
 * "<kind> <row> accept|refuse", a descriptor being accepted when both of its
 * parts pass; "fixed <kind> <row> ..." rows give the fixed part alone.
 * tests/test_field_resize.py holds the expected column.  Built with
 * AddressSanitizer + UBSan. */
#include <stdio.h>
#include <string.h>

#include "../broadway_amd/csrc/common/export_desc.h"

static void row(const char *kind, const char *name, int ok) { printf("%s %s %s\n", kind, name, ok ? "accept" : "refuse"); }

/* an accmv window (x, 0, cw, ch) of a w_mbs x h_mbs picture -> (oh, ow) */
static void accmv(const char *name, int w_mbs, int h_mbs, int x, int cw, int ch, int ow, int oh, int filter, int dtype, int nch)
{
    h264mi_accmv_resize_desc d;
    memset(&d, 0, sizeof(d));
    d.f.x = x; d.f.cw = cw; d.f.ch = ch; d.f.dtype = dtype; d.f.nch = nch;
    d.ow = ow; d.oh = oh; d.filter = filter;
    row("accmv", name, accmv_resize_fixed_ok(&d) && accmv_resize_window_ok(&d, w_mbs, h_mbs));
    printf("fixed accmv %s %s\n", name, accmv_resize_fixed_ok(&d) ? "accept" : "refuse");
}

static void accres(const char *name, int w_mbs, int h_mbs, int x, int cw, int ch, int ow, int oh, int filter, int dtype,
                   int planes, int colour, int unanchored)
{
    h264mi_accres_resize_desc d;
    memset(&d, 0, sizeof(d));
    d.f.x = x; d.f.cw = cw; d.f.ch = ch; d.f.dtype = dtype; d.f.planes = planes; d.f.colour = colour;
    d.f.unanchored = unanchored;
    d.ow = ow; d.oh = oh; d.filter = filter;
    row("accres", name, accres_resize_fixed_ok(&d) && accres_resize_window_ok(&d, w_mbs, h_mbs));
    printf("fixed accres %s %s\n", name, accres_resize_fixed_ok(&d) ? "accept" : "refuse");
}

int main(void)
{
    const int U8 = H264MI_TENSOR_U8, F16 = H264MI_TENSOR_F16, F32 = H264MI_TENSOR_F32, I16 = H264MI_TENSOR_I16;
    const int T = H264MI_RESIZE_TRIANGLE;
    const int Y = H264MI_ACCRES_Y, UV = H264MI_ACCRES_UV, RGB = H264MI_ACCRES_RGB;

    /* 6 x 4 MBs: 96 x 64 samples */
    accmv("identity", 6, 4, 0, 96, 64, 96, 64, T, I16, 2);
    accmv("down", 6, 4, 0, 96, 64, 37, 23, T, F16, 2);
    accmv("up", 6, 4, 5, 10, 6, 31, 17, T, F32, 8);
    accmv("ow_0", 6, 4, 0, 16, 16, 0, 8, T, I16, 2);
    accmv("ow_1", 6, 4, 0, 16, 16, 1, 8, T, I16, 2);
    accmv("ow_16384", 6, 4, 0, 16, 16, 16384, 8, T, I16, 2);
    accmv("ow_16385", 6, 4, 0, 16, 16, 16385, 8, T, I16, 2);
    accmv("oh_0", 6, 4, 0, 16, 16, 8, 0, T, I16, 2);
    accmv("oh_1", 6, 4, 0, 16, 16, 8, 1, T, I16, 2);
    accmv("oh_16384", 6, 4, 0, 16, 16, 8, 16384, T, I16, 2);
    accmv("oh_16385", 6, 4, 0, 16, 16, 8, 16385, T, I16, 2);
    accmv("ow_negative", 6, 4, 0, 16, 16, -1, 8, T, I16, 2);
    accmv("cw_32_ow", 6, 4, 0, 64, 16, 2, 8, T, I16, 2);
    accmv("cw_32_ow_plus_2", 6, 4, 0, 66, 16, 2, 8, T, I16, 2);
    accmv("ch_32_oh", 6, 4, 0, 16, 64, 8, 2, T, I16, 2);
    accmv("ch_32_oh_plus_1", 6, 4, 0, 16, 33, 8, 1, T, I16, 2);
    accmv("filter_1", 6, 4, 0, 16, 16, 8, 8, 1, I16, 2);
    accmv("filter_minus_1", 6, 4, 0, 16, 16, 8, 8, -1, I16, 2);
    accmv("dtype_u8", 6, 4, 0, 16, 16, 8, 8, T, U8, 2);
    accmv("nch_0", 6, 4, 0, 16, 16, 8, 8, T, I16, 0);
    accmv("nch_9", 6, 4, 0, 16, 16, 8, 8, T, I16, 9);
    accmv("window_past_the_picture", 6, 4, 90, 16, 16, 8, 8, T, I16, 2);
    accmv("cw_0", 6, 4, 0, 0, 16, 8, 8, T, I16, 2);
    /* 2048 x 1 MBs: a window may be 32768 wide, a resized one 16384 */
    accmv("grid_16384", 2048, 1, 0, 16384, 16, 512, 1, T, I16, 2);
    accmv("grid_16386", 2048, 1, 0, 16386, 16, 16384, 1, T, I16, 2);
    accmv("far_right", 2048, 1, 32704, 64, 16, 5, 3, T, I16, 2);

    accres("identity", 6, 4, 0, 96, 64, 96, 64, T, I16, Y, 0, 0);
    accres("rgb_down", 6, 4, 0, 96, 64, 37, 23, T, F16, RGB, 3, 1);
    accres("uv_identity", 6, 4, 0, 96, 64, 48, 32, T, I16, UV, 0, 0);
    accres("ow_0", 6, 4, 0, 16, 16, 0, 8, T, I16, Y, 0, 0);
    accres("ow_1", 6, 4, 0, 16, 16, 1, 8, T, I16, Y, 0, 0);
    accres("ow_16384", 6, 4, 0, 16, 16, 16384, 8, T, I16, Y, 0, 0);
    accres("ow_16385", 6, 4, 0, 16, 16, 16385, 8, T, I16, Y, 0, 0);
    accres("oh_16385", 6, 4, 0, 16, 16, 8, 16385, T, I16, Y, 0, 0);
    accres("cw_32_ow", 6, 4, 0, 64, 16, 2, 8, T, I16, Y, 0, 0);
    accres("cw_32_ow_plus_2", 6, 4, 0, 66, 16, 2, 8, T, I16, Y, 0, 0);
    accres("uv_cw_64_ow", 6, 4, 0, 64, 16, 1, 8, T, I16, UV, 0, 0);
    accres("uv_cw_64_ow_plus_2", 6, 4, 0, 66, 16, 1, 8, T, I16, UV, 0, 0);
    accres("uv_ch_64_oh", 6, 4, 0, 16, 64, 8, 1, T, I16, UV, 0, 0);
    accres("y_cw_64_ow", 6, 4, 0, 64, 16, 1, 8, T, I16, Y, 0, 0);
    accres("uv_odd_window", 6, 4, 0, 15, 16, 8, 8, T, I16, UV, 0, 0);
    accres("filter_1", 6, 4, 0, 16, 16, 8, 8, 1, I16, Y, 0, 0);
    accres("dtype_u8", 6, 4, 0, 16, 16, 8, 8, T, U8, Y, 0, 0);
    accres("planes_4", 6, 4, 0, 16, 16, 8, 8, T, I16, 4, 0, 0);
    accres("colour_4", 6, 4, 0, 16, 16, 8, 8, T, I16, RGB, 4, 0);
    accres("unanchored_2", 6, 4, 0, 16, 16, 8, 8, T, I16, Y, 0, 2);
    accres("window_past_the_picture", 6, 4, 90, 16, 16, 8, 8, T, I16, Y, 0, 0);
    /* UV of a window 32768 wide is a grid of 16384 */
    accres("uv_grid_16384", 2048, 1, 0, 32768, 16, 512, 1, T, I16, UV, 0, 0);
    accres("y_grid_16386", 2048, 1, 0, 16386, 16, 16384, 1, T, I16, Y, 0, 0);
    return 0;
}
