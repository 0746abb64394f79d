/* warp_desc_fixed_ok, warp_window_ok and warps_ok
 * (broadway_amd/csrc/common/export_desc.h), the rules of the affine-warped
 * export, walked over a small grid on NPICS pictures of 6 x 4 MBs (96 x 64 luma
 * samples): one line per row, "warp <row> accept|refuse".  A row is accepted
 * when all three rules hold, as the exports ask.  tests/test_warp_desc.py holds
 * the expected column.  Built with AddressSanitizer + UBSan. */
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include "../broadway_amd/csrc/common/export_desc.h"

enum { WIDTH = 96, HEIGHT = 64, NPICS = 3 };

static h264mi_tensor_warp_desc desc(void)
{
    h264mi_tensor_warp_desc d;
    memset(&d, 0, sizeof(d));
    d.t.cw = WIDTH; d.t.ch = HEIGHT;
    d.t.dtype = H264MI_TENSOR_F16;
    d.ow = 8; d.oh = 8; d.filter = H264MI_WARP_BILINEAR; d.border = H264MI_WARP_BORDER_CONSTANT;
    d.pad[0] = 114; d.pad[1] = 7; d.pad[2] = 250;
    d.layout = H264MI_LAYOUT_PLANAR;
    return d;
}

static const h264mi_warp kGood[4] = {{0, {65536, 0, 0, 0, 65536, 0}}, {1, {0, 0, 0, 0, 0, 0}},
                                     {2, {INT_MIN, INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX}},
                                     {0, {-65536, 0, 95 << 16, 0, -65536, 63 << 16}}};

static void row(const char *name, const h264mi_tensor_warp_desc *d, const h264mi_warp *w, int nwarps)
{
    printf("warp %s %s\n", name,
           warp_desc_fixed_ok(d) && warp_window_ok(d, WIDTH, HEIGHT) && warps_ok(w, nwarps, NPICS) ? "accept" : "refuse");
}

int main(void)
{
    h264mi_tensor_warp_desc d = desc();
    row("four_good", &d, kGood, 4);
    row("one_good", &d, kGood, 1);
    row("any_matrix", &d, kGood + 2, 1);
    row("nwarps_0", &d, kGood, 0);
    row("nwarps_negative", &d, kGood, -1);
    {
        h264mi_warp w[4];
        memcpy(w, kGood, sizeof(w));
        w[3].pic = NPICS - 1; row("pic_last", &d, w, 4);
        w[3].pic = NPICS; row("pic_npics_last", &d, w, 4);
        w[3].pic = -1; row("pic_minus_1_last", &d, w, 4);
    }
    /* the window: used, even, inside the picture */
    d = desc(); d.t.x = 6; d.t.y = 2; d.t.cw = 38; d.t.ch = 26; row("sub_window", &d, kGood, 4);
    d = desc(); d.t.x = 94; d.t.y = 62; d.t.cw = 2; d.t.ch = 2; row("window_2x2_far_corner", &d, kGood, 4);
    d = desc(); d.t.cw = 0; d.t.ch = 0; row("window_empty", &d, kGood, 4);
    d = desc(); d.t.x = 1; d.t.cw = 94; row("x_odd", &d, kGood, 4);
    d = desc(); d.t.y = 1; d.t.ch = 62; row("y_odd", &d, kGood, 4);
    d = desc(); d.t.cw = 95; row("cw_odd", &d, kGood, 4);
    d = desc(); d.t.ch = 63; row("ch_odd", &d, kGood, 4);
    d = desc(); d.t.x = 2; row("right_plus_2", &d, kGood, 4);
    d = desc(); d.t.y = 2; row("bottom_plus_2", &d, kGood, 4);
    d = desc(); d.t.x = -2; d.t.cw = 8; row("x_negative", &d, kGood, 4);
    d = desc(); d.t.ch = -2; row("ch_negative", &d, kGood, 4);
    /* the output size */
    d = desc(); d.ow = 1; d.oh = 1; row("size_1x1", &d, kGood, 4);
    d = desc(); d.ow = 16384; d.oh = 16384; row("size_max", &d, kGood, 4);
    d = desc(); d.ow = 0; row("ow_0", &d, kGood, 4);
    d = desc(); d.oh = 0; row("oh_0", &d, kGood, 4);
    d = desc(); d.ow = 16385; row("ow_max_plus_1", &d, kGood, 4);
    d = desc(); d.oh = 16385; row("oh_max_plus_1", &d, kGood, 4);
    /* filter, border, pad, layout, element type */
    d = desc(); d.filter = 1; row("filter_1", &d, kGood, 4);
    d = desc(); d.border = 2; row("border_2", &d, kGood, 4);
    d = desc(); d.border = -1; row("border_minus_1", &d, kGood, 4);
    d = desc(); d.pad[3] = 1; row("pad3_set", &d, kGood, 4);
    d = desc(); d.border = H264MI_WARP_BORDER_REPLICATE; row("replicate_with_pad", &d, kGood, 4);
    d = desc(); d.border = H264MI_WARP_BORDER_REPLICATE; d.pad[0] = d.pad[1] = 0; row("replicate_with_pad2", &d, kGood, 4);
    d = desc(); d.border = H264MI_WARP_BORDER_REPLICATE; memset(d.pad, 0, 4); row("replicate", &d, kGood, 4);
    d = desc(); d.layout = H264MI_LAYOUT_INTERLEAVED; row("interleaved", &d, kGood, 4);
    d = desc(); d.layout = 2; row("layout_2", &d, kGood, 4);
    d = desc(); d.t.dtype = H264MI_TENSOR_U8; row("dtype_u8", &d, kGood, 4);
    d = desc(); d.t.dtype = H264MI_TENSOR_F32; row("dtype_f32", &d, kGood, 4);
    d = desc(); d.t.dtype = H264MI_TENSOR_I16; row("dtype_i16", &d, kGood, 4);
    d = desc(); d.t.dtype = -1; row("dtype_minus_1", &d, kGood, 4);
    /* a side of the window beyond 16384, on a picture that holds it */
    d = desc(); d.t.cw = 16386; d.t.ch = 2;
    printf("warp window_16386 %s\n", warp_desc_fixed_ok(&d) && warp_window_ok(&d, 16400, 16) ? "accept" : "refuse");
    d.t.cw = 16384;
    printf("warp window_16384 %s\n", warp_desc_fixed_ok(&d) && warp_window_ok(&d, 16400, 16) ? "accept" : "refuse");
    printf("sizeof_warp %zu sizeof_desc %zu max_per_launch %d\n", sizeof(h264mi_warp), sizeof(h264mi_tensor_warp_desc),
           H264MI_WARPS_MAX_PER_LAUNCH);
    return 0;
}
