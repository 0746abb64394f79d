/* The descriptor rules of the device-tensor exports
 * (broadway_amd/csrc/common/export_desc.h) walked over a small grid on a 6 x 4
 * MB picture (96 x 64 luma samples, 24 x 16 blocks): one line per row, "<kind>
 * <row> accept|refuse", a descriptor being accepted when both of its parts
 * pass; then the crop-window helpers.  tests/test_export_desc.py holds the
 * expected column.  Built with AddressSanitizer + UBSan. */
#include <stdio.h>
#include <string.h>

#include "../broadway_amd/csrc/common/export_desc.h"

enum { W_MBS = 6, H_MBS = 4, WIDTH = 16 * W_MBS, HEIGHT = 16 * H_MBS };

static void row(const char *kind, const char *name, int ok) { printf("%s %s %s\n", kind, name, ok ? "accept" : "refuse"); }

static void tensor(const char *name, int x, int y, int cw, int ch, int dtype)
{
    h264mi_tensor_desc t;
    memset(&t, 0, sizeof(t));
    t.x = x; t.y = y; t.cw = cw; t.ch = ch; t.dtype = dtype;
    row("tensor", name, tensor_desc_fixed_ok(&t) && tensor_window_ok(&t, WIDTH, HEIGHT));
}

static void resize_on(const char *name, int width, int height, int x, int y, int cw, int ch, int dtype, int ow, int oh,
                      int filter)
{
    h264mi_tensor_resize_desc d;
    memset(&d, 0, sizeof(d));
    d.t.x = x; d.t.y = y; d.t.cw = cw; d.t.ch = ch; d.t.dtype = dtype;
    d.ow = ow; d.oh = oh; d.filter = filter;
    row("resize", name, resize_desc_fixed_ok(&d) && resize_window_ok(&d, width, height));
}

static void resize(const char *name, int x, int y, int cw, int ch, int dtype, int ow, int oh, int filter)
{
    resize_on(name, WIDTH, HEIGHT, x, y, cw, ch, dtype, ow, oh, filter);
}

static void mbinfo(const char *name, int bx, int by, int bw, int bh, int dtype, int nch, int last_ch)
{
    h264mi_mbinfo_desc d;
    memset(&d, 0, sizeof(d));
    d.bx = bx; d.by = by; d.bw = bw; d.bh = bh; d.dtype = dtype; d.nch = nch;
    if (nch >= 1 && nch <= H264MI_MBINFO_MAX_CH) d.ch[nch - 1] = last_ch;
    row("mbinfo", name, mbinfo_desc_fixed_ok(&d) && mbinfo_window_ok(&d, W_MBS, H_MBS));
}

static void residual(const char *name, int x, int y, int cw, int ch, int planes, int dtype)
{
    h264mi_residual_desc d;
    memset(&d, 0, sizeof(d));
    d.x = x; d.y = y; d.cw = cw; d.ch = ch; d.planes = planes; d.dtype = dtype;
    row("residual", name, residual_desc_fixed_ok(&d) && residual_window_ok(&d, W_MBS, H_MBS));
}

int main(void)
{
    const int U8 = H264MI_TENSOR_U8, F16 = H264MI_TENSOR_F16, BF16 = H264MI_TENSOR_BF16, F32 = H264MI_TENSOR_F32,
              I16 = H264MI_TENSOR_I16, TRI = H264MI_RESIZE_TRIANGLE;

    tensor("whole", 0, 0, 96, 64, F16);
    tensor("flush_right_bottom", 10, 20, 86, 44, F16);
    tensor("right_plus_1", 10, 20, 87, 44, F16);
    tensor("right_plus_2", 12, 20, 86, 44, F16);
    tensor("bottom_plus_1", 10, 20, 86, 45, F16);
    tensor("bottom_plus_2", 10, 22, 86, 44, F16);
    tensor("origin_0", 0, 0, 2, 2, F16);
    tensor("x_negative", -2, 0, 2, 2, F16);
    tensor("y_negative", 0, -2, 2, 2, F16);
    tensor("cw_0", 0, 0, 0, 2, F16);
    tensor("ch_0", 0, 0, 2, 0, F16);
    tensor("cw_negative", 4, 0, -2, 2, F16);
    tensor("ch_negative", 0, 4, 2, -2, F16);
    tensor("x_odd", 1, 0, 2, 2, F16);
    tensor("y_odd", 0, 1, 2, 2, F16);
    tensor("cw_odd", 0, 0, 3, 2, F16);
    tensor("ch_odd", 0, 0, 2, 3, F16);
    tensor("dtype_minus_1", 0, 0, 2, 2, -1);
    tensor("dtype_u8", 0, 0, 2, 2, U8);
    tensor("dtype_bf16", 0, 0, 2, 2, BF16);
    tensor("dtype_f32", 0, 0, 2, 2, F32);
    tensor("dtype_i16", 0, 0, 2, 2, I16);
    tensor("dtype_5", 0, 0, 2, 2, 5);

    resize("whole_half", 0, 0, 96, 64, F16, 48, 32, TRI);
    resize("flush_right_bottom", 10, 20, 86, 44, F16, 43, 22, TRI);
    resize("right_plus_1", 10, 20, 87, 44, F16, 43, 22, TRI);
    resize("right_plus_2", 12, 20, 86, 44, F16, 43, 22, TRI);
    resize("bottom_plus_1", 10, 20, 86, 45, F16, 43, 22, TRI);
    resize("bottom_plus_2", 10, 22, 86, 44, F16, 43, 22, TRI);
    resize("x_negative", -2, 0, 32, 32, F16, 8, 8, TRI);
    resize("y_negative", 0, -2, 32, 32, F16, 8, 8, TRI);
    resize("cw_0", 0, 0, 0, 32, F16, 8, 8, TRI);
    resize("ch_0", 0, 0, 32, 0, F16, 8, 8, TRI);
    resize("cw_negative", 4, 0, -2, 32, F16, 8, 8, TRI);
    resize("ch_negative", 0, 4, 32, -2, F16, 8, 8, TRI);
    resize("x_odd", 1, 0, 32, 32, F16, 8, 8, TRI);
    resize("y_odd", 0, 1, 32, 32, F16, 8, 8, TRI);
    resize("cw_odd", 0, 0, 31, 32, F16, 8, 8, TRI);
    resize("ch_odd", 0, 0, 32, 31, F16, 8, 8, TRI);
    resize("dtype_minus_1", 0, 0, 32, 32, -1, 8, 8, TRI);
    resize("dtype_u8", 0, 0, 32, 32, U8, 8, 8, TRI);
    resize("dtype_f32", 0, 0, 32, 32, F32, 8, 8, TRI);
    resize("dtype_i16", 0, 0, 32, 32, I16, 8, 8, TRI);
    resize("ow_0", 0, 0, 32, 32, F16, 0, 8, TRI);
    resize("ow_1", 0, 0, 32, 32, F16, 1, 8, TRI);
    resize("ow_16384", 0, 0, 32, 32, F16, 16384, 8, TRI);
    resize("ow_16385", 0, 0, 32, 32, F16, 16385, 8, TRI);
    resize("oh_0", 0, 0, 32, 32, F16, 8, 0, TRI);
    resize("oh_1", 0, 0, 32, 32, F16, 8, 1, TRI);
    resize("oh_16384", 0, 0, 32, 32, F16, 8, 16384, TRI);
    resize("oh_16385", 0, 0, 32, 32, F16, 8, 16385, TRI);
    resize("ow_negative", 0, 0, 32, 32, F16, -1, 8, TRI);
    resize("cw_32x", 0, 0, 64, 32, F16, 2, 8, TRI);
    resize("cw_32x_plus_2", 0, 0, 66, 32, F16, 2, 8, TRI);
    resize("ch_32x", 0, 0, 32, 64, F16, 8, 2, TRI);
    resize("ch_32x_plus_2", 0, 0, 32, 34, F16, 8, 1, TRI);
    resize("filter_1", 0, 0, 32, 32, F16, 8, 8, 1);
    resize("filter_minus_1", 0, 0, 32, 32, F16, 8, 8, -1);
    /* (the bound on cw and ch, which no 96 x 64 picture reaches) */
    resize_on("wide_cw_16384", 16400, 64, 0, 0, 16384, 32, F16, 16384, 8, TRI);
    resize_on("wide_cw_16386", 16400, 64, 0, 0, 16386, 32, F16, 16384, 8, TRI);
    resize_on("tall_ch_16384", 96, 16400, 0, 0, 32, 16384, F16, 8, 16384, TRI);
    resize_on("tall_ch_16386", 96, 16400, 0, 0, 32, 16386, F16, 8, 16384, TRI);

    mbinfo("whole", 0, 0, 24, 16, I16, 2, H264MI_MBINFO_MVY);
    mbinfo("flush_right_bottom", 3, 5, 21, 11, I16, 1, 0);
    mbinfo("right_plus_1", 3, 5, 22, 11, I16, 1, 0);
    mbinfo("right_plus_1_by_origin", 4, 5, 21, 11, I16, 1, 0);
    mbinfo("bottom_plus_1", 3, 5, 21, 12, I16, 1, 0);
    mbinfo("bottom_plus_1_by_origin", 3, 6, 21, 11, I16, 1, 0);
    mbinfo("origin_0", 0, 0, 1, 1, I16, 1, 0);
    mbinfo("odd_window", 1, 3, 5, 7, I16, 1, 0);
    mbinfo("bx_negative", -1, 0, 1, 1, I16, 1, 0);
    mbinfo("by_negative", 0, -1, 1, 1, I16, 1, 0);
    mbinfo("bw_0", 0, 0, 0, 1, I16, 1, 0);
    mbinfo("bh_0", 0, 0, 1, 0, I16, 1, 0);
    mbinfo("bw_negative", 2, 0, -1, 1, I16, 1, 0);
    mbinfo("bh_negative", 0, 2, 1, -1, I16, 1, 0);
    mbinfo("dtype_u8", 0, 0, 1, 1, U8, 1, 0);
    mbinfo("dtype_f16", 0, 0, 1, 1, F16, 1, 0);
    mbinfo("dtype_bf16", 0, 0, 1, 1, BF16, 1, 0);
    mbinfo("dtype_f32", 0, 0, 1, 1, F32, 1, 0);
    mbinfo("dtype_5", 0, 0, 1, 1, 5, 1, 0);
    mbinfo("dtype_minus_1", 0, 0, 1, 1, -1, 1, 0);
    mbinfo("nch_0", 0, 0, 1, 1, I16, 0, 0);
    mbinfo("nch_1", 0, 0, 1, 1, I16, 1, 0);
    mbinfo("nch_16", 0, 0, 1, 1, I16, 16, 0);
    mbinfo("nch_17", 0, 0, 1, 1, I16, 17, 0);
    mbinfo("nch_negative", 0, 0, 1, 1, I16, -1, 0);
    mbinfo("channel_minus_1", 0, 0, 1, 1, I16, 3, -1);
    mbinfo("channel_8", 0, 0, 1, 1, I16, 3, 8);
    mbinfo("channel_9", 0, 0, 1, 1, I16, 3, 9);
    mbinfo("channel_9_at_16", 0, 0, 1, 1, I16, 16, 9);

    static const struct { const char *name; int planes; } pl[] = {
        {"y", H264MI_RESID_Y}, {"uv", H264MI_RESID_UV}, {"yuv", H264MI_RESID_YUV}};
    for (int p = 0; p < 3; p++) {
        char name[64];
#define RESIDUAL(what, x, y, cw, ch, dtype)                        \
    do {                                                           \
        snprintf(name, sizeof(name), "%s_%s", pl[p].name, what);  \
        residual(name, x, y, cw, ch, pl[p].planes, dtype);         \
    } while (0)
        RESIDUAL("whole", 0, 0, 96, 64, I16);
        RESIDUAL("flush_right_bottom", 10, 20, 86, 44, I16);
        RESIDUAL("right_plus_1", 10, 20, 87, 44, I16);
        RESIDUAL("right_plus_2", 12, 20, 86, 44, I16);
        RESIDUAL("bottom_plus_1", 10, 20, 86, 45, I16);
        RESIDUAL("bottom_plus_2", 10, 22, 86, 44, I16);
        RESIDUAL("origin_0", 0, 0, 2, 2, I16);
        RESIDUAL("x_negative", -2, 0, 2, 2, I16);
        RESIDUAL("y_negative", 0, -2, 2, 2, I16);
        RESIDUAL("cw_0", 0, 0, 0, 2, I16);
        RESIDUAL("ch_0", 0, 0, 2, 0, I16);
        RESIDUAL("cw_negative", 4, 0, -2, 2, I16);
        RESIDUAL("ch_negative", 0, 4, 2, -2, I16);
        RESIDUAL("x_odd", 1, 0, 2, 2, I16);
        RESIDUAL("y_odd", 0, 1, 2, 2, I16);
        RESIDUAL("cw_odd", 0, 0, 3, 2, I16);
        RESIDUAL("ch_odd", 0, 0, 2, 3, I16);
        RESIDUAL("odd_flush", 1, 1, 95, 63, I16);
        RESIDUAL("dtype_u8", 0, 0, 2, 2, U8);
        RESIDUAL("dtype_f16", 0, 0, 2, 2, F16);
        RESIDUAL("dtype_bf16", 0, 0, 2, 2, BF16);
        RESIDUAL("dtype_f32", 0, 0, 2, 2, F32);
        RESIDUAL("dtype_5", 0, 0, 2, 2, 5);
        RESIDUAL("dtype_minus_1", 0, 0, 2, 2, -1);
#undef RESIDUAL
    }
    residual("planes_minus_1", 0, 0, 2, 2, -1, I16);
    residual("planes_3", 0, 0, 2, 2, 3, I16);

    /* crop_ltrb_6x4 of tests/golden/crop.json: 6, 4, 2 and 10 luma samples off
     * the left, right, top and bottom, in the SPS's units of 2 */
    export_window w = export_crop_window(W_MBS, H_MBS, 1, 3, 2, 1, 5), b = export_window_blocks(w);
    printf("crop ltrb %d %d %d %d blocks %d %d %d %d\n", w.x, w.y, w.cw, w.ch, b.x, b.y, b.cw, b.ch);
    /* without cropping the offsets mean nothing */
    w = export_crop_window(W_MBS, H_MBS, 0, 3, 2, 1, 5);
    b = export_window_blocks(w);
    printf("crop none %d %d %d %d blocks %d %d %d %d\n", w.x, w.y, w.cw, w.ch, b.x, b.y, b.cw, b.ch);
    printf("sizes %zu %zu %zu %zu %zu\n", export_elem_size(U8), export_elem_size(F16), export_elem_size(BF16),
           export_elem_size(F32), export_elem_size(I16));
    return 0;
}
