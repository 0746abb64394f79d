/* The fit and the rules of the letterboxed tensor export
 * (broadway_amd/csrc/common/export_desc.h) on the CPU:
 *   "fit <cw> <ch> <ow> <oh> <fit> <rw> <rh> <px> <py>"  letterbox_fit over a
 *       table of windows and canvases (tests/test_letterbox_desc.py holds the
 *       reference values, tests/test_letterbox_cpu.py compares the Python
 *       restatement with every line), then a pseudo-random sweep whose
 *       invariants are checked here ("sweep ok");
 *   "<kind> <row> accept|refuse"  fit_desc_fixed_ok + fit_window_ok ("fit_desc")
 *       and rois_fit_ok ("rois_fit") over a small grid on a 6 x 4 MB picture
 *       (96 x 64 luma samples).
 * Built with AddressSanitizer + UBSan. */
#include <stdio.h>
#include <string.h>

#include "../broadway_amd/csrc/common/export_desc.h"

enum { W_MBS = 6, H_MBS = 4, WIDTH = 16 * W_MBS, HEIGHT = 16 * H_MBS, NPICS = 3 };
enum { STRETCH = H264MI_FIT_STRETCH, BOX = H264MI_FIT_LETTERBOX, TOPLEFT = H264MI_FIT_LETTERBOX_TOPLEFT };

static void row(const char *kind, const char *name, int ok) { printf("%s %s %s\n", kind, name, ok ? "accept" : "refuse"); }

static void fit(int cw, int ch, int ow, int oh, int how)
{
    int f[4];
    letterbox_fit(cw, ch, ow, oh, how, f);
    printf("fit %d %d %d %d %d %d %d %d %d\n", cw, ch, ow, oh, how, f[0], f[1], f[2], f[3]);
}

static h264mi_tensor_fit_desc desc(int x, int y, int cw, int ch, int ow, int oh, int how, int pad3)
{
    h264mi_tensor_fit_desc d;
    memset(&d, 0, sizeof(d));
    d.r.t.x = x; d.r.t.y = y; d.r.t.cw = cw; d.r.t.ch = ch; d.r.t.dtype = H264MI_TENSOR_F16;
    d.r.ow = ow; d.r.oh = oh; d.r.filter = H264MI_RESIZE_TRIANGLE;
    d.fit = how;
    d.pad[0] = 114; d.pad[1] = 7; d.pad[2] = 250; d.pad[3] = (unsigned char)pad3;
    return d;
}

static void window(const char *name, int x, int y, int cw, int ch, int ow, int oh, int how, int pad3)
{
    const h264mi_tensor_fit_desc d = desc(x, y, cw, ch, ow, oh, how, pad3);
    int place[4];
    row("fit_desc", name, fit_desc_fixed_ok(&d) && fit_window_ok(&d, WIDTH, HEIGHT, place));
}

static void list(const char *name, const h264mi_roi *r, int nrois, int ow, int oh, int how, int pad3, int reserved_cw)
{
    const h264mi_tensor_fit_desc d = desc(0, 0, reserved_cw, 0, ow, oh, how, pad3);
    row("rois_fit", name, rois_fit_ok(&d, r, nrois, NPICS, WIDTH, HEIGHT));
}

int main(void)
{
    /* the reference values */
    fit(1920, 1080, 640, 640, BOX);
    fit(1920, 1080, 224, 224, BOX);
    fit(64, 128, 224, 224, BOX);
    fit(38, 26, 9, 7, BOX);
    /* 47 rows at exactly 32 : 1: nearest is 1 row, 47 source rows for one output; the rule raises it to 2 */
    fit(1504, 47, 47, 47, BOX);
    fit(47, 1504, 47, 47, BOX);
    /* the other modes, squares, up-scaling, a minor axis that rounds to 0, halves up, the largest sizes */
    fit(1920, 1080, 640, 640, TOPLEFT);
    fit(1920, 1080, 640, 640, STRETCH);
    fit(64, 128, 224, 224, TOPLEFT);
    fit(2, 2, 70, 40, BOX);
    fit(38, 26, 70, 40, BOX);
    fit(256, 32, 8, 3, BOX);
    fit(126, 32, 8, 3, BOX);
    fit(10, 26, 70, 20, TOPLEFT);
    fit(46, 10, 35, 37, TOPLEFT);
    fit(64, 2, 2, 2, BOX);
    fit(2, 64, 2, 2, BOX);
    fit(4, 2, 3, 3, BOX);
    fit(4, 6, 5, 5, BOX);
    fit(16384, 2, 16384, 16384, BOX);
    fit(2, 16384, 16384, 16384, BOX);
    fit(16384, 16384, 16384, 1, BOX);
    fit(16384, 16382, 16383, 16384, BOX);
    fit(86, 52, 30, 40, BOX);
    fit(86, 52, 1280, 2, BOX);

    /* a sweep (a 64-bit LCG): even cw, ch <= 16384, ow, oh <= 2048; where the
     * major axis is within 32 : 1 the content lies inside the canvas and
     * both axes are within 32 : 1 */
    unsigned long long s = 0x9E3779B97F4A7C15ull;
    int n = 0, bad = 0;
    for (int k = 0; k < 200000; k++) {
        int v[4];
        for (int i = 0; i < 4; i++) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            v[i] = (int)(s >> 40);
        }
        const int cw = 2 + 2 * (v[0] % 8192), ch = 2 + 2 * (v[1] % 8192), ow = 1 + v[2] % 2048, oh = 1 + v[3] % 2048;
        const int wide = (long long)cw * oh >= (long long)ch * ow;
        if (wide ? cw > 32 * ow : ch > 32 * oh) continue;
        int f[4];
        letterbox_fit(cw, ch, ow, oh, BOX, f);
        n++;
        if (f[0] < 1 || f[0] > ow || f[1] < 1 || f[1] > oh || cw > 32 * f[0] || ch > 32 * f[1] || f[2] != (ow - f[0]) / 2 ||
            f[3] != (oh - f[1]) / 2 || (wide ? f[0] != ow : f[1] != oh)) {
            if (!bad++) printf("sweep bad %d %d %d %d -> %d %d %d %d\n", cw, ch, ow, oh, f[0], f[1], f[2], f[3]);
        }
    }
    printf("sweep %s\n", n > 100000 && !bad ? "ok" : "failed");

    /* the single-window rules */
    window("whole_letterbox", 0, 0, 96, 64, 8, 8, BOX, 0);
    window("whole_topleft", 0, 0, 96, 64, 8, 8, TOPLEFT, 0);
    window("whole_stretch", 0, 0, 96, 64, 8, 8, STRETCH, 0);
    window("fit_3", 0, 0, 96, 64, 8, 8, 3, 0);
    window("fit_minus_1", 0, 0, 96, 64, 8, 8, -1, 0);
    window("pad3_set", 0, 0, 96, 64, 8, 8, BOX, 1);
    window("pad3_set_stretch", 0, 0, 96, 64, 8, 8, STRETCH, 255);
    window("major_32x", 0, 0, 96, 2, 3, 3, BOX, 0);
    window("major_32x_plus_2", 0, 0, 96, 2, 2, 3, BOX, 0);              /* 96 columns into 2 */
    window("major_32x_tall", 0, 0, 2, 64, 5, 2, BOX, 0);
    window("major_32x_plus_2_tall", 0, 0, 2, 64, 5, 1, BOX, 0);         /* 64 rows into 1 */
    window("minor_kept_by_the_raise", 0, 0, 96, 34, 3, 3, BOX, 0);      /* nearest 1 row; raised to 2 */
    window("stretch_33x", 0, 0, 96, 64, 8, 1, STRETCH, 0);              /* 64 rows into 1 */
    window("letterbox_of_the_same", 0, 0, 96, 64, 8, 1, BOX, 0);        /* height-bound: 64 rows into 1 */
    window("stretch_minor_33x", 0, 0, 96, 2, 2, 3, STRETCH, 0);
    window("upscaled", 4, 6, 2, 2, 70, 40, BOX, 0);
    window("x_odd", 1, 0, 16, 16, 8, 8, BOX, 0);
    window("cw_odd", 0, 0, 15, 16, 8, 8, BOX, 0);
    window("right_plus_2", 12, 20, 86, 44, 8, 8, BOX, 0);
    window("cw_0", 0, 0, 0, 16, 8, 8, BOX, 0);
    window("ow_0", 0, 0, 96, 64, 0, 8, BOX, 0);
    window("oh_16385", 0, 0, 96, 64, 8, 16385, BOX, 0);

    /* lists */
    const h264mi_roi good[4] = {{0, 0, 0, 96, 64}, {1, 10, 20, 86, 44}, {2, 4, 6, 2, 2}, {0, 2, 2, 16, 48}};
    h264mi_roi l[4];
    for (int how = STRETCH; how <= TOPLEFT; how++) {
        char name[32];
        snprintf(name, sizeof(name), "four_good_fit_%d", how);
        list(name, good, 4, 8, 8, how, 0, 0);
    }
    list("fit_3", good, 4, 8, 8, 3, 0, 0);
    list("pad3_set", good, 4, 8, 8, BOX, 1, 0);
    list("reserved_window_set", good, 4, 8, 8, BOX, 0, 2);
    list("nrois_0", good, 0, 8, 8, BOX, 0, 0);
    memcpy(l, good, sizeof(l)); l[3].x = 3;
    list("bad_box_last_odd", l, 4, 8, 8, BOX, 0, 0);
    memcpy(l, good, sizeof(l)); l[1].pic = NPICS;
    list("bad_box_pic", l, 4, 8, 8, BOX, 0, 0);
    memcpy(l, good, sizeof(l)); l[2].cw = 4; l[2].x = 94;
    list("bad_box_over_the_edge", l, 4, 8, 8, BOX, 0, 0);
    list("one_box_beyond_32x", good, 4, 2, 8, BOX, 0, 0);               /* boxes 0 and 1 are wider than 64 */
    list("tall_box_beyond_32x_stretched", good, 4, 8, 1, STRETCH, 0, 0);
    list("tall_box_beyond_32x", good, 4, 8, 1, BOX, 0, 0);              /* height-bound: 64 rows into 1 */
    list("all_within_32x", good, 4, 3, 2, BOX, 0, 0);

    printf("sizeof_fit_desc %zu fits %d %d %d\n", sizeof(h264mi_tensor_fit_desc), STRETCH, BOX, TOPLEFT);
    return 0;
}
