/* Which bytes of a reference slot a macroblock's motion compensation reads,
 * stated once.  Plain C11 / C++17, no HIP: k_wgpp's dependency checker
 * (recon_kernels.hip chk_ref_rows) walks the accesses from here, the host
 * takes its MbRec.i4 encoding and its line count from here (host/capture.c),
 * and tests/mc_window_check.cpp proves every function against a brute-force
 * list of the touched bytes.  The loads (mc_issue) and the column-granular
 * wait (dep_wait_cols) do NOT take anything from here: they spell the same
 * windows, rows, lane map and mcw_span_cells out by hand, because taken from
 * here they compiled to slower code.  For them this header is
 * a proven specification, kept in step by hand: a change here is a change in
 * both.  The checker verifies the wait and the host encoding against this
 * header; nothing but a comment ties mc_issue's loads to it, and the check
 * program restates dep_wait_cols' branches against mcw_span_cells on the CPU
 * only (tests/mc_window_check.cpp dep_wait_cols_rule: a copy of the kernel's
 * lines, not the kernel's code).
 *
 * A slot (H264MI_SLOT_BYTES) is a luma plane with rows W16 = 16 w bytes apart,
 * then Cb and Cr with rows H264MI_CPITCH apart.  Every plane's size is a
 * multiple of 128, so no 128-B line holds bytes of two planes, and a chroma
 * line holds bytes of one row; a luma line holds the end of earlier rows
 * when W16 % 128 != 0.
 *
 * The window of 4x4 block b (z-scan) with quarter-pel MV (mvx, mvy):
 *   luma    9 rows of 12 bytes, chroma (per component) 3 rows of 8 bytes;
 *   x0, y0  its first sample, unclamped (luma: the 6-tap filter's 2 to the
 *           left and above);
 *   ax      the column the loads start at: x0 rounded down to a dword and
 *           clamped so that the load stays in the row.  The 9 (3) columns
 *           clamp(x0 + i, 0, width - 1) the interpolation reads all lie in
 *           [ax, ax + 11] ([ax, ax + 7]): mc_finish picks them from there;
 *   row k   at clamp(y0 + k, 0, rows - 1). */
#ifndef H264MI_MC_WINDOW_H
#define H264MI_MC_WINDOW_H

#include <stdint.h>
#include "../../../include/h264mi_records.h"

/* always_inline, like the kernel's own __forceinline__ helpers */
#ifdef __cplusplus
#define MCW_FN static inline __attribute__((always_inline)) constexpr   /* host and device under hipcc */
#else
#define MCW_FN static inline __attribute__((always_inline))
#endif

enum { MCW_LUMA_ROWS = 9, MCW_LUMA_BYTES = 12, MCW_CHROMA_ROWS = 3, MCW_CHROMA_BYTES = 8, MCW_LINE = 128 };

MCW_FN int mcw_min(int a, int b) { return a < b ? a : b; }
MCW_FN int mcw_max(int a, int b) { return a > b ? a : b; }
MCW_FN int mcw_clamp(int lo, int hi, int v) { return mcw_min(mcw_max(v, lo), hi); }
MCW_FN int mcw_div(int a, int b) { return (int)((uint32_t)a / (uint32_t)b); }      /* of non-negative values */
/* 4x4 block b of an MB in z-scan: its column and row in blocks; its 8x8 partition (MbRec.ref, MbRec.i4) */
MCW_FN int mcw_blk_x(int b) { return ((b >> 2) & 1) * 2 + (b & 1); }
MCW_FN int mcw_blk_y(int b) { return ((b >> 3) & 1) * 2 + ((b >> 1) & 1); }
MCW_FN int mcw_blk_part(int b) { return b >> 2; }

/* A plane of a w x h MB picture's slot: first byte, row pitch, rows, bytes
 * per row in use, and an MB's rows and bytes per row in it */
typedef struct { uint32_t base; int pitch, rows, width, mbh, mbw; } mcw_plane;

MCW_FN mcw_plane mcw_luma_plane(int w, int h)
{
    const mcw_plane p = {0u, w * 16, h * 16, w * 16, 16, 16};
    return p;
}
MCW_FN mcw_plane mcw_chroma_plane(int w, int h, int comp)
{
    const mcw_plane y = mcw_luma_plane(w, h);       /* half its rows and width, behind it */
    const mcw_plane p = {(uint32_t)(y.pitch * y.rows) + (uint32_t)(comp * H264MI_CPITCH(w) * (y.rows / 2)),
                         H264MI_CPITCH(w), y.rows / 2, y.width / 2, 8, 8};
    return p;
}
MCW_FN int mcw_row(const mcw_plane *pl, int y) { return mcw_clamp(0, pl->rows - 1, y); }

typedef struct { int x0, y0, ax; } mcw_win;

MCW_FN mcw_win mcw_luma(int w, int mbx, int mby, int b, int mvx, int mvy)
{
    const int x0 = mbx * 16 + mcw_blk_x(b) * 4 + (mvx >> 2) - 2;
    const mcw_win r = {x0, mby * 16 + mcw_blk_y(b) * 4 + (mvy >> 2) - 2, mcw_clamp(0, w * 16 - MCW_LUMA_BYTES, x0 & ~3)};
    return r;
}
MCW_FN mcw_win mcw_chroma(int w, int mbx, int mby, int b, int mvx, int mvy)
{
    const int x0 = mbx * 8 + mcw_blk_x(b) * 2 + (mvx >> 3);
    const mcw_win r = {x0, mby * 8 + mcw_blk_y(b) * 2 + (mvy >> 3), mcw_clamp(0, w * 16 / 2 - MCW_CHROMA_BYTES, x0 & ~3)};
    return r;
}

/* mc_issue's lane map: a wave of 64 loads every window of an MB.
 * Luma: lane -> block lane >> 2, window rows min((lane & 3) + 4k, 8) for
 * k = 0..2.  Chroma: lane -> block (lane & 31) >> 1, component lane & 1,
 * window rows (lane >> 5) + {0, 1}.  The waits and the checker hold a lane
 * to luma rows (lane & 3)..8 and chroma rows 0..2 of its blocks. */
enum { MCW_LANES = 64, MCW_LANE_LUMA_LOADS = 3, MCW_LANE_CHROMA_LOADS = 2 };
MCW_FN int mcw_lane_luma_blk(int lane) { return lane >> 2; }
MCW_FN int mcw_lane_luma_first(int lane) { return lane & 3; }
MCW_FN int mcw_lane_luma_row(int lane, int k) { return mcw_min(mcw_lane_luma_first(lane) + 4 * k, MCW_LUMA_ROWS - 1); }
MCW_FN int mcw_lane_chroma_blk(int lane) { return (lane & 31) >> 1; }
MCW_FN int mcw_lane_chroma_comp(int lane) { return lane & 1; }
MCW_FN int mcw_lane_chroma_row(int lane, int k) { return (lane >> 5) + k; }

/* What the 128-B lines of an access hold: MB rows r_lo..r_hi of the plane,
 * through MB column x.  An access is len bytes from column x of row y. */
typedef struct { int r_lo, r_hi, x; } mcw_cells;

MCW_FN int mcw_one_row_lines(const mcw_plane *pl) { return pl->pitch % MCW_LINE == 0; }
MCW_FN mcw_cells mcw_access_cells(const mcw_plane *pl, int x, int len, int y)
{
    const uint32_t o = (uint32_t)(y * pl->pitch + x), pitch = (uint32_t)pl->pitch;
    const uint32_t ls = o & ~(uint32_t)(MCW_LINE - 1), le = (o + len - 1) | (MCW_LINE - 1);
    const int ya = (int)(ls / pitch), yb = (int)(le / pitch);
    /* lines that hold a row's end hold that row's last column */
    const mcw_cells r = {mcw_div(ya, pl->mbh), mcw_div(yb, pl->mbh),
                         mcw_div(ya == yb ? mcw_min((int)(le % pitch), pl->width - 1) : pl->width - 1, pl->mbw)};
    return r;
}
/* the accesses of rows ya..yb (clamped) at column x together, without a walk
 * over the rows: r_lo and r_hi are those of the first and last access; x is
 * theirs where a line holds one row, and otherwise the plane's last column,
 * which a line that holds a row's end needs (an upper bound where none of
 * the lines does) */
MCW_FN mcw_cells mcw_span_cells(const mcw_plane *pl, int x, int len, int ya, int yb)
{
    if (mcw_one_row_lines(pl)) {
        const mcw_cells r = {mcw_div(ya, pl->mbh), mcw_div(yb, pl->mbh),
                             mcw_div(mcw_min((x + len - 1) | (MCW_LINE - 1), pl->width - 1), pl->mbw)};
        return r;
    }
    const mcw_cells r = {mcw_access_cells(pl, x, len, ya).r_lo, mcw_access_cells(pl, x, len, yb).r_hi,
                         mcw_div(pl->width - 1, pl->mbw)};
    return r;
}

/* MbRec.i4 of an inter MB at (mbx, mby): per 8x8 partition the last MB row of
 * its reference slot that a line read by its blocks' windows touches
 * (recon_kernels.hip dep_wait_rows waits for it).  An access's r_hi -- the MB
 * row of its last line's last byte -- grows with its row: a window's last
 * row is the one that counts. */
static inline void mcw_ref_rows(const MbRec *r, int w, int h, int mbx, int mby, uint16_t rows[4])
{
    const mcw_plane yp = mcw_luma_plane(w, h), cp = mcw_chroma_plane(w, h, 0);     /* Cr: the same rows */
    rows[0] = rows[1] = rows[2] = rows[3] = 0;
    for (int b = 0; b < 16; b++) {
        const mcw_win l = mcw_luma(w, mbx, mby, b, r->mv[b][0], r->mv[b][1]);
        const mcw_win c = mcw_chroma(w, mbx, mby, b, r->mv[b][0], r->mv[b][1]);
        const int n = mcw_max(mcw_access_cells(&yp, l.ax, MCW_LUMA_BYTES, mcw_row(&yp, l.y0 + MCW_LUMA_ROWS - 1)).r_hi,
                              mcw_access_cells(&cp, c.ax, MCW_CHROMA_BYTES, mcw_row(&cp, c.y0 + MCW_CHROMA_ROWS - 1)).r_hi);
        if (n > rows[mcw_blk_part(b)]) rows[mcw_blk_part(b)] = (uint16_t)n;
    }
}

/* Every access of block b of an inter MB, as offsets into its reference slot:
 * the luma window's rows (MCW_LUMA_BYTES each), then the Cb and the Cr
 * window's (MCW_CHROMA_BYTES each) */
enum { MCW_BLK_ACCESSES = MCW_LUMA_ROWS + 2 * MCW_CHROMA_ROWS };
MCW_FN int mcw_blk_access_len(int j) { return j < MCW_LUMA_ROWS ? MCW_LUMA_BYTES : MCW_CHROMA_BYTES; }
static inline void mcw_blk_accesses(const MbRec *r, int w, int h, int mbx, int mby, int b, uint32_t off[MCW_BLK_ACCESSES])
{
    const mcw_plane yp = mcw_luma_plane(w, h);
    const mcw_win l = mcw_luma(w, mbx, mby, b, r->mv[b][0], r->mv[b][1]);
    const mcw_win c = mcw_chroma(w, mbx, mby, b, r->mv[b][0], r->mv[b][1]);
    for (int k = 0; k < MCW_LUMA_ROWS; k++) *off++ = yp.base + (uint32_t)(mcw_row(&yp, l.y0 + k) * yp.pitch + l.ax);
    for (int comp = 0; comp < 2; comp++) {
        const mcw_plane cp = mcw_chroma_plane(w, h, comp);
        for (int k = 0; k < MCW_CHROMA_ROWS; k++) *off++ = cp.base + (uint32_t)(mcw_row(&cp, c.y0 + k) * cp.pitch + c.ax);
    }
}

#ifdef __cplusplus
static_assert(mcw_blk_x(6) == 2 && mcw_blk_y(6) == 1 && mcw_blk_x(9) == 1 && mcw_blk_y(9) == 2, "z-scan");
static_assert(mcw_lane_luma_row(63, 2) == MCW_LUMA_ROWS - 1 && mcw_lane_luma_row(60, 1) == 4, "luma rows 0..8");
static_assert(mcw_lane_chroma_row(63, MCW_LANE_CHROMA_LOADS - 1) == MCW_CHROMA_ROWS - 1, "chroma rows 0..2");
static_assert(mcw_luma_plane(9, 5).pitch % MCW_LINE != 0 && mcw_chroma_plane(9, 5, 1).pitch % MCW_LINE == 0, "");
static_assert(mcw_chroma_plane(9, 5, 1).base + (uint32_t)(H264MI_CPITCH(9) * 40) == H264MI_SLOT_BYTES(9, 5), "");
#endif

#endif
