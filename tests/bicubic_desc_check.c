/* The rules of H264MI_RESIZE_BICUBIC in
 * broadway_amd/csrc/common/export_desc.h on the CPU -- the filters that exist,
 * and 16 source samples per output and axis where the triangle takes 32 --
 * through every descriptor that carries a filter: one line per row, on pictures
 * of 32 x 4 MBs (512 x 64),
 *   bicubic <name> accept|refuse
 * tests/test_bicubic_cpu.py builds this with AddressSanitizer + UBSan and
 * compares the lines with its written-out table. */
#include "../broadway_amd/csrc/common/export_desc.h"

#include <stdio.h>
#include <string.h>

#define W 512
#define H 64
#define T H264MI_RESIZE_TRIANGLE
#define B H264MI_RESIZE_BICUBIC

static void row(const char *name, int ok) { printf("bicubic %s %s\n", name, ok ? "accept" : "refuse"); }

/* the window (0, 0, cw, ch) into ow x oh under `filter` and `fit` */
static h264mi_tensor_layout_desc desc(int cw, int ch, int ow, int oh, int filter, int fit)
{
    h264mi_tensor_layout_desc d;
    memset(&d, 0, sizeof(d));
    d.f.r.t.cw = cw; d.f.r.t.ch = ch;
    d.f.r.t.mode = H264MI_TENSOR_RGB;
    d.f.r.t.dtype = H264MI_TENSOR_F16;
    d.f.r.ow = ow; d.f.r.oh = oh; d.f.r.filter = filter;
    d.f.fit = fit;
    d.layout = H264MI_LAYOUT_INTERLEAVED;
    return d;
}

static void resize_row(const char *name, int cw, int ch, int ow, int oh, int filter)
{
    const h264mi_tensor_layout_desc d = desc(cw, ch, ow, oh, filter, H264MI_FIT_STRETCH);
    row(name, resize_desc_fixed_ok(&d.f.r) && resize_window_ok(&d.f.r, W, H));
}

static void fit_row(const char *name, int cw, int ch, int ow, int oh, int filter, int fit)
{
    const h264mi_tensor_layout_desc d = desc(cw, ch, ow, oh, filter, fit);
    row(name, fit_desc_fixed_ok(&d.f) && fit_window_ok(&d.f, W, H, NULL));
}

static void layout_row(const char *name, int cw, int ch, int ow, int oh, int filter, int fit)
{
    const h264mi_tensor_layout_desc d = desc(cw, ch, ow, oh, filter, fit);
    row(name, layout_desc_fixed_ok(&d) && layout_window_ok(&d, W, H));
}

/* a list of two boxes, the first cw x ch, over two pictures */
static void list_row(const char *name, int cw, int ch, int ow, int oh, int filter, int fit, int form)
{
    const h264mi_roi boxes[2] = {{0, 0, 0, cw, ch}, {1, 4, 6, 32, 32}};
    const h264mi_tensor_layout_desc d = desc(0, 0, ow, oh, filter, fit);
    row(name, form == 0 ? rois_ok(&d.f.r, boxes, 2, 2, W, H) : form == 1 ? rois_fit_ok(&d.f, boxes, 2, 2, W, H)
                                                             : rois_layout_ok(&d, boxes, 2, 2, W, H));
}

static void field_row(const char *name, int filter)
{
    h264mi_accmv_resize_desc m;
    h264mi_accres_resize_desc r;
    char full[64];
    memset(&m, 0, sizeof(m));
    memset(&r, 0, sizeof(r));
    m.f.cw = 96; m.f.ch = 64; m.f.dtype = H264MI_TENSOR_I16; m.f.nch = 2;
    m.ow = 9; m.oh = 7; m.filter = filter;
    r.f.cw = 96; r.f.ch = 64; r.f.dtype = H264MI_TENSOR_I16; r.f.planes = H264MI_ACCRES_Y;
    r.ow = 9; r.oh = 7; r.filter = filter;
    snprintf(full, sizeof(full), "accmv_%s", name);
    row(full, accmv_resize_fixed_ok(&m) && accmv_resize_window_ok(&m, W / 16, H / 16));
    snprintf(full, sizeof(full), "accres_%s", name);
    row(full, accres_resize_fixed_ok(&r) && accres_resize_window_ok(&r, W / 16, H / 16));
}

int main(void)
{
    const int S = H264MI_FIT_STRETCH, L = H264MI_FIT_LETTERBOX;

    /* the filters */
    resize_row("filter_bicubic", 96, 64, 9, 7, B);
    resize_row("filter_triangle", 96, 64, 9, 7, T);
    resize_row("filter_1", 96, 64, 9, 7, 1);
    resize_row("filter_minus_1", 96, 64, 9, 7, -1);
    resize_row("filter_3", 96, 64, 9, 7, 3);
    fit_row("fit_filter_bicubic", 96, 64, 9, 7, B, L);
    fit_row("fit_filter_1", 96, 64, 9, 7, 1, L);
    fit_row("fit_filter_3", 96, 64, 9, 7, 3, L);
    layout_row("layout_filter_bicubic", 96, 64, 9, 7, B, S);
    layout_row("layout_filter_3", 96, 64, 9, 7, 3, S);
    layout_row("layout_unresized_filter_bicubic", 96, 64, 0, 0, B, S);
    layout_row("layout_unresized_filter_0", 96, 64, 0, 0, T, S);
    list_row("rois_filter_bicubic", 96, 64, 9, 7, B, S, 0);
    list_row("rois_filter_1", 96, 64, 9, 7, 1, S, 0);
    list_row("rois_filter_3", 96, 64, 9, 7, 3, S, 0);

    /* 16 : 1 and beyond, per axis */
    resize_row("bicubic_cw_16_ow", 256, 64, 16, 7, B);
    resize_row("bicubic_cw_16_ow_plus_2", 258, 64, 16, 7, B);
    resize_row("triangle_cw_16_ow_plus_2", 258, 64, 16, 7, T);
    resize_row("bicubic_ch_16_oh", 96, 64, 9, 4, B);
    resize_row("bicubic_ch_16_oh_plus_2", 96, 50, 9, 3, B);
    resize_row("triangle_ch_16_oh_plus_2", 96, 50, 9, 3, T);
    resize_row("triangle_cw_32_ow", 512, 64, 16, 7, T);
    resize_row("bicubic_cw_32_ow", 512, 64, 16, 7, B);
    resize_row("bicubic_upscale", 2, 2, 64, 64, B);
    fit_row("fit_bicubic_cw_16_ow", 256, 64, 16, 7, B, S);
    fit_row("fit_bicubic_cw_16_ow_plus_2", 258, 64, 16, 7, B, S);
    fit_row("fit_triangle_cw_16_ow_plus_2", 258, 64, 16, 7, T, S);
    /* letterboxed into 20 x 20: 320 x 40 is (20, 3) -- 40 rows to 3 --, 320 x 34 is (20, 2): the shared fit raises
     * the minor axis to ceil(34 / 32) only, 17 rows per output */
    fit_row("letterbox_bicubic_minor_within_16", 320, 40, 20, 20, B, L);
    fit_row("letterbox_bicubic_minor_beyond_16", 320, 34, 20, 20, B, L);
    fit_row("letterbox_triangle_minor_beyond_16", 320, 34, 20, 20, T, L);
    fit_row("letterbox_bicubic_major_beyond_16", 322, 40, 20, 20, B, L);
    layout_row("layout_bicubic_cw_16_ow_plus_2", 258, 64, 16, 7, B, S);
    layout_row("layout_letterbox_bicubic_minor_beyond_16", 320, 34, 20, 20, B, L);
    list_row("rois_bicubic_cw_16_ow", 256, 64, 16, 7, B, S, 0);
    list_row("rois_bicubic_cw_16_ow_plus_2", 258, 64, 16, 7, B, S, 0);
    list_row("rois_triangle_cw_16_ow_plus_2", 258, 64, 16, 7, T, S, 0);
    list_row("rois_fit_bicubic_minor_within_16", 320, 40, 20, 20, B, L, 1);
    list_row("rois_fit_bicubic_minor_beyond_16", 320, 34, 20, 20, B, L, 1);
    list_row("rois_fit_triangle_minor_beyond_16", 320, 34, 20, 20, T, L, 1);
    list_row("rois_layout_bicubic_cw_16_ow", 256, 64, 16, 7, B, S, 2);
    list_row("rois_layout_bicubic_cw_16_ow_plus_2", 258, 64, 16, 7, B, S, 2);

    /* the field exports have the triangle only */
    field_row("filter_triangle", T);
    field_row("filter_bicubic", B);

    {
        int f[4];
        letterbox_fit(320, 34, 20, 20, L, f);
        printf("fit_320x34_into_20x20 %d %d %d %d\n", f[0], f[1], f[2], f[3]);
    }
    printf("enum triangle %d bicubic %d\n", H264MI_RESIZE_TRIANGLE, H264MI_RESIZE_BICUBIC);
    return 0;
}
