/* The rules of h264mi_tensor_layout_desc, layout_desc_fixed_ok /
 * layout_window_ok / rois_layout_ok in broadway_amd/csrc/common/export_desc.h,
 * on the CPU: one line per row, on pictures of 6 x 4 MBs (96 x 64),
 *   layout <name> accept|refuse
 * tests/test_layout_desc.py builds this with AddressSanitizer + UBSan and
 * compares the lines with its written-out table. */
#include "../broadway_amd/csrc/common/export_desc.h"

#include <stdio.h>
#include <string.h>

#define W 96
#define H 64

/* the unresized export of the whole picture, planar */
static h264mi_tensor_layout_desc plain(void)
{
    h264mi_tensor_layout_desc d;
    memset(&d, 0, sizeof(d));
    d.f.r.t.cw = W; d.f.r.t.ch = H;
    d.f.r.t.mode = H264MI_TENSOR_RGB;
    d.f.r.t.dtype = H264MI_TENSOR_F16;
    d.layout = H264MI_LAYOUT_PLANAR;
    return d;
}

/* the same window into 9 x 7 */
static h264mi_tensor_layout_desc sized(int fit)
{
    h264mi_tensor_layout_desc d = plain();
    d.f.r.ow = 9; d.f.r.oh = 7; d.f.r.filter = H264MI_RESIZE_TRIANGLE;
    d.f.fit = fit;
    return d;
}

/* for a list: the window reserved */
static h264mi_tensor_layout_desc listed(int fit)
{
    h264mi_tensor_layout_desc d = sized(fit);
    d.f.r.t.cw = d.f.r.t.ch = 0;
    return d;
}

static void window_row(const char *name, h264mi_tensor_layout_desc d)
{
    printf("layout %s %s\n", name, layout_desc_fixed_ok(&d) && layout_window_ok(&d, W, H) ? "accept" : "refuse");
}

static void list_row(const char *name, h264mi_tensor_layout_desc d, const h264mi_roi *r, int n)
{
    printf("layout %s %s\n", name, rois_layout_ok(&d, r, n, 3, W, H) ? "accept" : "refuse");
}

int main(void)
{
    static const h264mi_roi boxes[2] = {{0, 0, 0, 96, 64}, {2, 4, 6, 2, 2}}, bad[2] = {{0, 0, 0, 96, 64}, {3, 4, 6, 2, 2}};
    h264mi_tensor_layout_desc d;

    window_row("plain_planar", plain());
    d = plain(); d.layout = H264MI_LAYOUT_INTERLEAVED; window_row("plain_interleaved", d);
    d = plain(); d.layout = 2; window_row("plain_layout_2", d);
    d = plain(); d.layout = -1; window_row("plain_layout_minus_1", d);
    d = plain(); d.f.r.t.mode = H264MI_TENSOR_GRAY; d.layout = H264MI_LAYOUT_INTERLEAVED; window_row("plain_gray_interleaved", d);
    d = plain(); d.f.fit = H264MI_FIT_LETTERBOX; window_row("plain_fit_letterbox", d);
    d = plain(); d.f.fit = H264MI_FIT_LETTERBOX_TOPLEFT; window_row("plain_fit_topleft", d);
    d = plain(); d.f.pad[0] = 114; window_row("plain_pad0", d);
    d = plain(); d.f.pad[2] = 1; window_row("plain_pad2", d);
    d = plain(); d.f.pad[3] = 1; window_row("plain_pad3", d);
    d = plain(); d.f.r.filter = 1; window_row("plain_filter_1", d);
    d = plain(); d.f.r.ow = 9; window_row("only_oh_0", d);
    d = plain(); d.f.r.oh = 7; window_row("only_ow_0", d);
    d = plain(); d.f.r.t.dtype = H264MI_TENSOR_I16; window_row("plain_dtype_i16", d);
    d = plain(); d.f.r.t.x = 1; window_row("plain_x_odd", d);
    d = plain(); d.f.r.t.cw = W + 2; window_row("plain_too_wide", d);

    window_row("stretch_planar", sized(H264MI_FIT_STRETCH));
    d = sized(H264MI_FIT_STRETCH); d.layout = H264MI_LAYOUT_INTERLEAVED; window_row("stretch_interleaved", d);
    d = sized(H264MI_FIT_LETTERBOX); d.layout = H264MI_LAYOUT_INTERLEAVED; d.f.pad[0] = 114; d.f.pad[1] = 7; d.f.pad[2] = 250;
    window_row("letterbox_interleaved", d);
    d = sized(H264MI_FIT_LETTERBOX_TOPLEFT); window_row("topleft_planar", d);
    d = sized(H264MI_FIT_LETTERBOX); d.layout = 2; window_row("letterbox_layout_2", d);
    d = sized(H264MI_FIT_LETTERBOX); d.f.pad[3] = 1; window_row("letterbox_pad3", d);
    d = sized(3); window_row("fit_3", d);
    d = sized(H264MI_FIT_STRETCH); d.f.r.filter = 1; window_row("stretch_filter_1", d);
    d = sized(H264MI_FIT_STRETCH); d.f.r.oh = 1; window_row("stretch_beyond_32x", d);         /* 64 rows to 1 */
    d = sized(H264MI_FIT_STRETCH); d.f.r.ow = 16385; window_row("stretch_ow_16385", d);

    d = listed(H264MI_FIT_STRETCH); d.layout = H264MI_LAYOUT_INTERLEAVED; list_row("boxes_stretch_interleaved", d, boxes, 2);
    list_row("boxes_letterbox_planar", listed(H264MI_FIT_LETTERBOX), boxes, 2);
    d = listed(H264MI_FIT_STRETCH); d.f.r.ow = d.f.r.oh = 0; list_row("boxes_no_size", d, boxes, 2);
    d = listed(H264MI_FIT_STRETCH); d.f.r.oh = 0; list_row("boxes_only_oh_0", d, boxes, 2);
    list_row("boxes_window_set", sized(H264MI_FIT_STRETCH), boxes, 2);
    d = listed(H264MI_FIT_LETTERBOX); d.f.r.t.x = 2; list_row("boxes_window_x_set", d, boxes, 2);
    d = listed(H264MI_FIT_STRETCH); d.layout = 2; list_row("boxes_layout_2", d, boxes, 2);
    list_row("boxes_nrois_0", listed(H264MI_FIT_STRETCH), boxes, 0);
    list_row("boxes_bad_pic_last", listed(H264MI_FIT_STRETCH), bad, 2);

    printf("sizeof_layout_desc %zu fit_desc %zu\n", sizeof(h264mi_tensor_layout_desc), sizeof(h264mi_tensor_fit_desc));
    return 0;
}
