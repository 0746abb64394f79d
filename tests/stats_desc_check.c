/* The rules of h264mi_stats_desc, stats_desc_fixed_ok,
 * stats_window_ok, stats_rois_ok and stats_item_words in
 * broadway_amd/csrc/common/export_desc.h, on the CPU: one line per row,
 *   desc <name> accept|refuse          a descriptor with its own window, on a 64 x 48 picture
 *   rois <name> accept|refuse          a descriptor and a box list over 3 pictures of 64 x 48
 *   words <planes> <flags> <P * L>
 * tests/test_stats_desc.py builds this with AddressSanitizer + UBSan and
 * compares the lines with its written-out table. */
#include "../broadway_amd/csrc/common/export_desc.h"

#include <limits.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#define W 64
#define H 48
#define NPICS 3

static h264mi_stats_desc desc(int x, int y, int cw, int ch, int planes, int colour, int flags)
{
    h264mi_stats_desc d;
    memset(&d, 0, sizeof(d));
    d.x = x; d.y = y; d.cw = cw; d.ch = ch; d.planes = planes; d.colour = colour; d.flags = flags;
    return d;
}

static void row_of(const char *name, const h264mi_stats_desc *d)
{
    printf("desc %s %s\n", name, stats_desc_fixed_ok(d) && stats_window_ok(d, W, H) ? "accept" : "refuse");
}

static void rois_of(const char *name, const h264mi_stats_desc *d, const h264mi_roi *r, int n)
{
    printf("rois %s %s\n", name, stats_rois_ok(d, r, n, NPICS, W, H) ? "accept" : "refuse");
}

int main(void)
{
    h264mi_stats_desc d;

    d = desc(0, 0, W, H, H264MI_STATS_Y, 0, 0); row_of("whole_y", &d);
    d = desc(0, 0, W, H, H264MI_STATS_YUV, 0, H264MI_STATS_HIST); row_of("whole_yuv_hist", &d);
    d = desc(0, 0, W, H, H264MI_STATS_RGB, 0, 0); row_of("whole_rgb", &d);
    d = desc(0, 0, W, H, H264MI_STATS_RGB, 3, H264MI_STATS_HIST); row_of("rgb_colour_3", &d);
    d = desc(6, 2, 38, 26, H264MI_STATS_Y, 0, 0); row_of("sub_window", &d);
    d = desc(62, 46, 2, 2, H264MI_STATS_YUV, 0, 0); row_of("last_2x2", &d);
    d = desc(2, 0, 62, 48, H264MI_STATS_RGB, 1, 0); row_of("x_2_mod_4", &d);

    d = desc(0, 0, W, H, 3, 0, 0); row_of("planes_3", &d);
    d = desc(0, 0, W, H, -1, 0, 0); row_of("planes_minus_1", &d);
    d = desc(0, 0, W, H, H264MI_STATS_Y, 0, 2); row_of("flag_2", &d);
    d = desc(0, 0, W, H, H264MI_STATS_Y, 0, -1); row_of("flags_all", &d);
    d = desc(0, 0, W, H, H264MI_STATS_Y, 0, 0); d.reserved = 1; row_of("reserved_1", &d);
    d = desc(0, 0, W, H, H264MI_STATS_Y, 1, 0); row_of("colour_with_y", &d);
    d = desc(0, 0, W, H, H264MI_STATS_YUV, 2, 0); row_of("colour_with_yuv", &d);
    d = desc(0, 0, W, H, H264MI_STATS_RGB, 4, 0); row_of("colour_4", &d);
    d = desc(0, 0, W, H, H264MI_STATS_RGB, -1, 0); row_of("colour_minus_1", &d);
    d = desc(0, 0, W, H, H264MI_STATS_RGB, H264MI_TENSOR_COLOUR_STREAM, 0); row_of("colour_stream", &d);
    d = desc(1, 0, 38, 26, H264MI_STATS_Y, 0, 0); row_of("x_odd", &d);
    d = desc(0, 1, 38, 26, H264MI_STATS_Y, 0, 0); row_of("y_odd", &d);
    d = desc(0, 0, 37, 26, H264MI_STATS_Y, 0, 0); row_of("cw_odd", &d);
    d = desc(0, 0, 38, 25, H264MI_STATS_Y, 0, 0); row_of("ch_odd", &d);
    d = desc(0, 0, 0, H, H264MI_STATS_Y, 0, 0); row_of("cw_0", &d);
    d = desc(0, 0, W, 0, H264MI_STATS_Y, 0, 0); row_of("ch_0", &d);
    d = desc(-2, 0, 38, 26, H264MI_STATS_Y, 0, 0); row_of("x_negative", &d);
    d = desc(0, -2, 38, 26, H264MI_STATS_Y, 0, 0); row_of("y_negative", &d);
    d = desc(28, 0, 38, 26, H264MI_STATS_Y, 0, 0); row_of("past_right", &d);
    d = desc(0, 24, 38, 26, H264MI_STATS_Y, 0, 0); row_of("past_bottom", &d);
    d = desc(2, 2, INT_MAX - 1, 2, H264MI_STATS_Y, 0, 0); row_of("cw_huge", &d);
    d = desc(INT_MAX - 1, 2, 2, 2, H264MI_STATS_Y, 0, 0); row_of("x_huge", &d);

    {
        const h264mi_stats_desc z = desc(0, 0, 0, 0, H264MI_STATS_RGB, 2, H264MI_STATS_HIST);
        const h264mi_roi good[4] = {{0, 0, 0, W, H}, {2, 6, 2, 38, 26}, {1, 62, 46, 2, 2}, {2, 6, 2, 38, 26}};
        rois_of("good", &z, good, 4);
        rois_of("one_box", &z, good, 1);
        rois_of("none", &z, good, 0);
        rois_of("minus_1", &z, good, -1);
        d = z; d.cw = 2; d.ch = 2; rois_of("with_a_window", &d, good, 4);
        d = z; d.x = 2; rois_of("with_a_window_x", &d, good, 4);
        d = z; d.planes = 3; rois_of("bad_planes", &d, good, 4);
        d = z; d.planes = H264MI_STATS_Y; rois_of("colour_with_y", &d, good, 4);
        d = z; d.reserved = 4; rois_of("reserved_4", &d, good, 4);
        h264mi_roi b[4];
        memcpy(b, good, sizeof(b)); b[3].pic = NPICS; rois_of("last_pic_3", &z, b, 4);
        memcpy(b, good, sizeof(b)); b[0].pic = -1; rois_of("first_pic_minus_1", &z, b, 4);
        memcpy(b, good, sizeof(b)); b[2].x = 61; rois_of("box_x_odd", &z, b, 4);
        memcpy(b, good, sizeof(b)); b[2].cw = 4; rois_of("box_past_right", &z, b, 4);
        memcpy(b, good, sizeof(b)); b[1].ch = 48; rois_of("box_past_bottom", &z, b, 4);
        memcpy(b, good, sizeof(b)); b[3].ch = 0; rois_of("last_box_empty", &z, b, 4);
        memcpy(b, good, sizeof(b)); b[1].cw = 37; rois_of("box_cw_odd", &z, b, 4);
    }

    for (int planes = H264MI_STATS_Y; planes <= H264MI_STATS_RGB; planes++)
        for (int flags = 0; flags <= H264MI_STATS_HIST; flags++) {
            d = desc(0, 0, 0, 0, planes, 0, flags);
            printf("words %d %d %zu\n", planes, flags, stats_item_words(&d));
        }
    d = desc(0, 0, 0, 0, 3, 0, 0); printf("words bad_planes %zu\n", stats_item_words(&d));
    d = desc(0, 0, 0, 0, H264MI_STATS_Y, 0, 2); printf("words bad_flags %zu\n", stats_item_words(&d));

    printf("sizeof_desc %zu planes %zu colour %zu flags %zu reserved %zu\n", sizeof(h264mi_stats_desc),
           offsetof(h264mi_stats_desc, planes), offsetof(h264mi_stats_desc, colour), offsetof(h264mi_stats_desc, flags),
           offsetof(h264mi_stats_desc, reserved));
    return 0;
}
