/* The rules of h264mi_tensor_dest, dest_ok in
 * broadway_amd/csrc/common/export_desc.h, on the CPU: one line per row,
 *   dest <name> accept|refuse
 * over items of 3 x 32 x 48 fp16 elements (es = 2) unless the row says
 * otherwise: a packed row is 96 bytes (interleaved: 288), a packed plane 3072,
 * a packed item 9216.  tests/test_dest_desc.py builds this with
 * AddressSanitizer + UBSan and compares the lines with its written-out table. */
#include "../broadway_amd/csrc/common/export_desc.h"

#include <stddef.h>
#include <stdio.h>
#include <string.h>

#define ES 2
#define P 3
#define ROWS 32
#define COLS 48
#define ROW (COLS * ES)             /* 96 */
#define PLANE (ROWS * ROW)          /* 3072 */
#define ITEM (P * PLANE)            /* 9216 */

static h264mi_tensor_dest dest(int64_t row, int64_t plane, int64_t frame, int clip)
{
    h264mi_tensor_dest d;
    memset(&d, 0, sizeof(d));
    d.row = row; d.plane = plane; d.frame = frame; d.clip = clip;
    return d;
}

static void row_of(const char *name, const h264mi_tensor_dest *d, int interleaved, int nitems, size_t out_stride)
{
    printf("dest %s %s\n", name, dest_ok(d, ES, P, ROWS, COLS, interleaved, nitems, out_stride) ? "accept" : "refuse");
}

int main(void)
{
    h264mi_tensor_dest d;

    row_of("null", NULL, 0, 3, ITEM);
    row_of("null_interleaved", NULL, 1, 3, ITEM);
    d = dest(0, 0, 0, 1); row_of("all_zero", &d, 0, 3, ITEM);
    d = dest(0, 0, 0, 1); row_of("all_zero_interleaved", &d, 1, 3, ITEM);
    d = dest(ROW, PLANE, 0, 1); row_of("explicit_contiguous", &d, 0, 3, ITEM);
    d = dest(3 * ROW, 0, 0, 1); row_of("explicit_contiguous_interleaved", &d, 1, 3, ITEM);
    /* (N, C, T, H, W) with T = 3, six items: two clips */
    d = dest(0, 3 * PLANE, PLANE, 3); row_of("ncthw", &d, 0, 6, 3 * 3 * PLANE);
    d = dest(ROW + 16, ROWS * (ROW + 16), 0, 1); row_of("row_padded_16", &d, 0, 3, P * ROWS * (ROW + 16));
    d = dest(ROW + ES, 0, 0, 1); row_of("row_padded_one_element", &d, 0, 3, P * ROWS * (ROW + ES));
    /* channels 1..3 of an (N, 5, H, W) tensor: items 5 planes apart */
    d = dest(0, 0, 0, 1); row_of("channel_slice", &d, 0, 3, 5 * PLANE);
    /* clip.permute(1, 0, 2, 3) of a (C, T, H, W) clip as (T, C, H, W): the item stride below the plane stride */
    d = dest(0, 3 * PLANE, 0, 1); row_of("permuted_clip", &d, 0, 3, PLANE);
    /* a 2 x 4 grid of tiles in one (C, 2 * 32, 4 * 48) canvas: the frame (a tile to the right) below the row */
    d = dest(4 * ROW, 2 * ROWS * 4 * ROW, ROW, 4); row_of("tile_grid", &d, 0, 8, ROWS * 4 * ROW);
    d = dest(4 * 3 * ROW, 0, 3 * ROW, 4); row_of("tile_grid_interleaved", &d, 1, 8, ROWS * 4 * 3 * ROW);
    d = dest(0, 0, 0, 1); row_of("one_item_any_out_stride", &d, 0, 1, 2);

    d = dest(ROW + 1, 0, 0, 1); row_of("row_not_multiple_of_es", &d, 0, 1, 0);
    d = dest(0, PLANE + 1, 0, 1); row_of("plane_not_multiple_of_es", &d, 0, 1, 0);
    d = dest(0, 0, ITEM + 1, 3); row_of("frame_not_multiple_of_es", &d, 0, 3, 0);
    d = dest(0, 0, 0, 1); row_of("out_stride_not_multiple_of_es", &d, 0, 3, ITEM + 1);
    d = dest(ROW - ES, 0, 0, 1); row_of("row_one_element_short", &d, 0, 3, ITEM);
    d = dest(3 * ROW - ES, 0, 0, 1); row_of("row_one_element_short_interleaved", &d, 1, 3, ITEM);
    d = dest(0, PLANE, 0, 1); row_of("plane_set_interleaved", &d, 1, 3, ITEM);
    d = dest(0, PLANE - ES, 0, 1); row_of("plane_overlaps_last_row", &d, 0, 3, ITEM);
    d = dest(0, 0, ITEM - ES, 3); row_of("frame_overlaps", &d, 0, 3, 3 * ITEM);
    d = dest(0, 0, 0, 3); row_of("frame_zero_in_clip", &d, 0, 3, 3 * ITEM);
    d = dest(0, 0, 0, 1); row_of("out_stride_overlaps", &d, 0, 3, ITEM - ES);
    d = dest(0, 0, 0, 1); row_of("out_stride_zero", &d, 0, 3, 0);
    d = dest(0, 3 * PLANE, PLANE, 3); row_of("ncthw_clips_overlap", &d, 0, 6, 3 * 3 * PLANE - ES);
    d = dest(0, 0, 0, 0); row_of("clip_0", &d, 0, 3, ITEM);
    d = dest(0, 0, 0, -1); row_of("clip_minus_1", &d, 0, 3, ITEM);
    d = dest(0, 3 * PLANE, PLANE, 3); row_of("nitems_not_multiple_of_clip", &d, 0, 7, 3 * 3 * PLANE);
    d = dest(0, 0, ITEM, 1); row_of("frame_set_clip_1", &d, 0, 3, ITEM);
    d = dest(0, 0, 0, 1); d.reserved = 1; row_of("reserved_1", &d, 0, 3, ITEM);
    d = dest(-ROW, 0, 0, 1); row_of("row_negative", &d, 0, 3, ITEM);
    d = dest(0, -PLANE, 0, 1); row_of("plane_negative", &d, 0, 3, ITEM);
    d = dest(0, 0, -ITEM, 3); row_of("frame_negative", &d, 0, 3, 3 * ITEM);
    /* the tiles of the grid one element too close: the second tile's rows run into the first's */
    d = dest(4 * ROW, 2 * ROWS * 4 * ROW, ROW - ES, 4); row_of("tile_grid_tiles_overlap", &d, 0, 8, ROWS * 4 * ROW);
    /* spans beyond 63 bits are refused, not wrapped */
    d = dest(0, INT64_MAX - 1, 0, 1); row_of("plane_span_overflows", &d, 0, 3, ITEM);
    d = dest(INT64_MAX - 1, 0, 0, 1); row_of("row_span_overflows", &d, 0, 3, ITEM);     /* rows * row, before it is formed */
    d = dest(INT64_MAX / ROWS - 1, 0, 0, 1); row_of("row_span_overflows_late", &d, 0, 3, ITEM);     /* fits, its span does not */

    printf("sizeof_dest %zu row %zu plane %zu frame %zu clip %zu reserved %zu\n", sizeof(h264mi_tensor_dest),
           offsetof(h264mi_tensor_dest, row), offsetof(h264mi_tensor_dest, plane), offsetof(h264mi_tensor_dest, frame),
           offsetof(h264mi_tensor_dest, clip), offsetof(h264mi_tensor_dest, reserved));
    return 0;
}
