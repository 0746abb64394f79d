/* rois_ok (broadway_amd/csrc/common/export_desc.h), the rule of the
 * region-of-interest export, walked over a small grid on NPICS pictures of 6 x
 * 4 MBs (96 x 64 luma samples): one line per row, "rois <row> accept|refuse".
 * tests/test_rois_desc.py holds the expected column.  Built with
 * AddressSanitizer + UBSan. */
#include <stdio.h>
#include <string.h>

#include "../broadway_amd/csrc/common/export_desc.h"

enum { WIDTH = 96, HEIGHT = 64, NPICS = 3 };

static h264mi_tensor_resize_desc desc(int ow, int oh)
{
    h264mi_tensor_resize_desc d;
    memset(&d, 0, sizeof(d));
    d.t.dtype = H264MI_TENSOR_F16;
    d.ow = ow; d.oh = oh; d.filter = H264MI_RESIZE_TRIANGLE;
    return d;
}

static void row(const char *name, const h264mi_tensor_resize_desc *d, const h264mi_roi *r, int nrois)
{
    printf("rois %s %s\n", name, rois_ok(d, r, nrois, NPICS, WIDTH, HEIGHT) ? "accept" : "refuse");
}

/* one box to (ow, oh) = (8, 8) */
static void one(const char *name, int pic, int x, int y, int cw, int ch)
{
    const h264mi_tensor_resize_desc d = desc(8, 8);
    const h264mi_roi r = {pic, x, y, cw, ch};
    row(name, &d, &r, 1);
}

int main(void)
{
    one("whole", 0, 0, 0, 96, 64);
    one("flush_right_bottom", 1, 10, 20, 86, 44);
    one("box_2x2", 0, 4, 6, 2, 2);
    one("pic_last", NPICS - 1, 0, 0, 16, 16);
    one("pic_npics", NPICS, 0, 0, 16, 16);
    one("pic_minus_1", -1, 0, 0, 16, 16);
    one("x_odd", 0, 1, 0, 16, 16);
    one("y_odd", 0, 0, 1, 16, 16);
    one("cw_odd", 0, 0, 0, 15, 16);
    one("ch_odd", 0, 0, 0, 16, 15);
    one("right_plus_1", 1, 10, 20, 87, 44);
    one("right_plus_2", 1, 12, 20, 86, 44);
    one("bottom_plus_1", 1, 10, 20, 86, 45);
    one("bottom_plus_2", 1, 10, 22, 86, 44);
    one("cw_0", 0, 0, 0, 0, 16);
    one("ch_negative", 0, 0, 4, 16, -2);

    /* 32 source samples per output and axis: 64 -> 2, and 2 more */
    {
        const h264mi_tensor_resize_desc d = desc(2, 8), e = desc(8, 1);
        const h264mi_roi a = {0, 0, 0, 64, 32}, b = {0, 0, 0, 66, 32}, c = {0, 0, 0, 32, 32}, f = {0, 0, 0, 32, 34};
        row("cw_32x", &d, &a, 1);
        row("cw_32x_plus_2", &d, &b, 1);
        row("ch_32x", &e, &c, 1);
        row("ch_32x_plus_2", &e, &f, 1);
    }
    /* upscaling */
    {
        const h264mi_tensor_resize_desc d = desc(64, 48);
        const h264mi_roi a = {2, 2, 2, 2, 2};
        row("upscaled", &d, &a, 1);
    }
    /* the list: none, a negative count, the reserved window, a bad output size, one bad box last among good ones */
    {
        h264mi_tensor_resize_desc d = desc(8, 8);
        const h264mi_roi good[4] = {{0, 0, 0, 96, 64}, {1, 10, 20, 86, 44}, {2, 4, 6, 2, 2}, {0, 2, 2, 16, 16}};
        h264mi_roi last_bad[4];
        memcpy(last_bad, good, sizeof(good));
        last_bad[3].x = 3;
        row("four_good", &d, good, 4);
        row("nrois_0", &d, good, 0);
        row("nrois_negative", &d, good, -1);
        row("bad_box_last", &d, last_bad, 4);
        d.t.cw = 96; d.t.ch = 64;
        row("reserved_window_set", &d, good, 4);
        d = desc(8, 8); d.t.x = 2;
        row("reserved_x_set", &d, good, 4);
        d = desc(8, 8); d.t.y = 2;
        row("reserved_y_set", &d, good, 4);
        d = desc(0, 8);
        row("ow_0", &d, good, 4);
        d = desc(8, 8); d.filter = 1;
        row("filter_1", &d, good, 4);
        d = desc(8, 8); d.t.dtype = H264MI_TENSOR_I16;
        row("dtype_i16", &d, good, 4);
    }
    printf("sizeof_roi %zu max_per_launch %d\n", sizeof(h264mi_roi), H264MI_ROIS_MAX_PER_LAUNCH);
    return 0;
}
