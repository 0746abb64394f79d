// The MC reference-window geometry (broadway_amd/csrc/common/mc_window.h)
// against a brute-force list of the bytes a window touches.  The rule is
// restated here on its own (window(): which samples the interpolation of a
// 4x4 block needs and which bytes the loads fetch), every byte
// of a slot is mapped to its (plane, MB row, MB column) cell, and every
// 128-B line to the cells of its bytes; nothing below takes a window, a row,
// a line or a cell from the header except to compare it.
//
// Picture sizes cover W16 % 128 zero and non-zero, CW < 128, CP > CW and
// W16 - 12 = 4; MBs at the corners, the edges and inside; every block; MVs
// that leave the picture by more than a window on every side and hit every
// fractional phase.  Integer work, no tolerance.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "../broadway_amd/csrc/common/mc_window.h"

static long long g_bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_bad++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const int BX[16] = {0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3};
static const int BY[16] = {0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3};
static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

struct Cells { int r_lo, r_hi, x; };
static void merge(Cells &a, const Cells &b)
{
    a.r_lo = std::min(a.r_lo, b.r_lo); a.r_hi = std::max(a.r_hi, b.r_hi); a.x = std::max(a.x, b.x);
}

// A slot of a w x h MB picture, byte by byte
struct Slot {
    int w, h, W16, H16, CW, CH, CP;
    size_t ysz, csz, bytes;
    std::vector<Cells> line;        // per 128-B line: the cells of its bytes (r_lo > r_hi: none)
    std::vector<int> line_plane;    // and their plane (0 Y, 1 Cb, 2 Cr; -1: padding only)
    std::vector<char> line_rows2;   // whether it holds bytes of two sample rows

    Slot(int w_, int h_) : w(w_), h(h_), W16(w_ * 16), H16(h_ * 16), CW(w_ * 8), CH(h_ * 8), CP((w_ * 8 + 127) / 128 * 128)
    {
        ysz = (size_t)W16 * H16; csz = (size_t)CP * CH; bytes = ysz + 2 * csz;
        line.assign(bytes / 128, Cells{1 << 30, -1, -1});
        line_plane.assign(bytes / 128, -1);
        line_rows2.assign(bytes / 128, 0);
        for (size_t o = 0; o < bytes; o++) {
            int pl, r, c;
            if (!cell(o, pl, r, c)) continue;
            if (o % 128 && o < ysz && o % W16 == 0) line_rows2[o / 128] = 1;
            CHECK(line_plane[o / 128] < 0 || line_plane[o / 128] == pl, "line %zu holds two planes", o / 128);
            line_plane[o / 128] = pl;
            merge(line[o / 128], Cells{r, r, c});
        }
        // (MB rows start 256 w bytes apart: a line can hold the end of an
        // earlier sample row, never of an earlier MB row)
        for (const Cells &c : line) CHECK(c.r_lo >= c.r_hi, "a line holds two MB rows");
    }
    // plane, MB row and MB column of slot byte o; false: chroma row padding
    bool cell(size_t o, int &pl, int &r, int &c) const
    {
        if (o < ysz) { pl = 0; r = (int)(o / W16) / 16; c = (int)(o % W16) / 16; return true; }
        o -= ysz; pl = 1 + (int)(o / csz); o %= csz;
        if ((int)(o % CP) >= CW) return false;
        r = (int)(o / CP) / 8; c = (int)(o % CP) / 8;
        return true;
    }
    // slot byte of sample (x, y) of a plane (coordinates inside it)
    size_t at(int pl, int x, int y) const
    {
        return pl == 0 ? (size_t)y * W16 + x : ysz + (size_t)(pl - 1) * csz + (size_t)y * CP + x;
    }
    // the cells of the lines that bytes [o, o + len) touch
    Cells cells_of(size_t o, int len) const
    {
        Cells c{1 << 30, -1, -1};
        for (int i = 0; i < len; i++) merge(c, line[(o + i) / 128]);
        return c;
    }
};

// The rule, restated.  Block b of MB (mbx, mby) with quarter-pel MV: the
// interpolation reads luma samples (x0 + i, y0 + k), i, k = 0..8, chroma
// (x0 + i, y0 + k), i, k = 0..2, each coordinate clamped to the plane; the
// loads fetch per row 12 (8) bytes from the dword at or below x0, moved
// inside the row.
struct Win { int x0, y0, ax, n, len, width, rows; };
static Win window(const Slot &s, int pl, int mbx, int mby, int b, int mvx, int mvy)
{
    Win v;
    if (pl == 0) {
        v.x0 = mbx * 16 + BX[b] * 4 + (mvx >> 2) - 2; v.y0 = mby * 16 + BY[b] * 4 + (mvy >> 2) - 2;
        v.n = 9; v.len = 12; v.width = s.W16; v.rows = s.H16;
    } else {
        v.x0 = mbx * 8 + BX[b] * 2 + (mvx >> 3); v.y0 = mby * 8 + BY[b] * 2 + (mvy >> 3);
        v.n = 3; v.len = 8; v.width = s.CW; v.rows = s.CH;
    }
    v.ax = clampi(v.x0 & ~3, 0, v.width - v.len);
    return v;
}

static const int SIZES[][2] = {{1, 1}, {2, 1}, {1, 2}, {3, 2}, {5, 4}, {8, 3}, {9, 5}, {13, 7}, {22, 6}, {120, 3}};

// MV components: every phase & 7 of both signs, a few samples to tens of
// samples, and beyond the far edge from any MB by more than a window
static std::vector<int> mv_axis(int dim)
{
    std::vector<int> v;
    for (int i = -9; i <= 9; i++) v.push_back(i);
    for (int i : {52, 132, (dim + 29) * 4 + 3, (dim + 29) * 4 + 6}) { v.push_back(i); v.push_back(-i); }
    return v;
}

static long long n_windows = 0, n_accesses = 0, n_clamped = 0, n_two_rows = 0;

// dep_wait_cols (recon_kernels.hip) does not call the header: it spells the
// lane's rows lsub..8 (chroma 0..2) and mcw_span_cells' two branches out.
// This is a copy of those lines (min / max / clip3 as there), compared with
// mcw_span_cells below -- a copy, not the kernel's code: it shows that the
// lines as they stood when copied state the header's rule, and has to be
// kept in step with the kernel by hand.
static int clip3(int lo, int hi, int v) { return std::min(std::max(v, lo), hi); }
static Cells dep_wait_cols_rule(int w, int h, bool chroma, int mbx, int mby, int b, int mvx, int mvy, int lsub)
{
    const int W16 = w * 16, H16 = h * 16, CW = W16 / 2, CH = H16 / 2;
    Cells c;
    if (!chroma) {
        const int x0 = clip3(0, W16 - 12, (mbx * 16 + BX[b] * 4 + (mvx >> 2) - 2) & ~3);
        const int y0 = mby * 16 + BY[b] * 4 + (mvy >> 2) - 2;
        const int ya = clip3(0, H16 - 1, y0 + lsub), yb = clip3(0, H16 - 1, y0 + 8);
        if ((W16 & 127) == 0) {
            c.r_lo = ya >> 4; c.r_hi = yb >> 4;
            c.x = std::min((x0 + 11) | 127, W16 - 1) >> 4;
        } else {
            const uint32_t ls = ((uint32_t)ya * W16 + x0) & ~127u, le = ((uint32_t)yb * W16 + x0 + 11) | 127u;
            c.r_lo = (int)(ls / (uint32_t)W16) >> 4;
            c.r_hi = std::min((int)(le / (uint32_t)W16), H16 - 1) >> 4;
            c.x = w - 1;
        }
    } else {
        const int x0 = clip3(0, CW - 8, (mbx * 8 + BX[b] * 2 + (mvx >> 3)) & ~3);
        const int y0 = mby * 8 + BY[b] * 2 + (mvy >> 3);
        c.r_lo = clip3(0, CH - 1, y0) >> 3; c.r_hi = clip3(0, CH - 1, y0 + 2) >> 3;
        c.x = std::min((x0 + 7) | 127, CW - 1) >> 3;
    }
    return c;
}

static void check_window(const Slot &s, int mbx, int mby, int b, int mvx, int mvy)
{
    const mcw_plane planes[3] = {mcw_luma_plane(s.w, s.h), mcw_chroma_plane(s.w, s.h, 0), mcw_chroma_plane(s.w, s.h, 1)};
    for (int pl = 0; pl < 3; pl++) {
        const Win v = window(s, pl, mbx, mby, b, mvx, mvy);
        const mcw_win hw = pl == 0 ? mcw_luma(s.w, mbx, mby, b, mvx, mvy) : mcw_chroma(s.w, mbx, mby, b, mvx, mvy);
        const mcw_plane *hp = &planes[pl];
        n_windows++;
        CHECK(hw.x0 == v.x0 && hw.y0 == v.y0 && hw.ax == v.ax, "window %dx%d mb %d,%d b %d mv %d,%d plane %d", s.w, s.h, mbx, mby, b, mvx, mvy, pl);
        CHECK(hp->base == s.at(pl, 0, 0) && hp->rows == v.rows && hp->width == v.width && hp->pitch == (pl ? s.CP : s.W16), "plane %d", pl);
        CHECK((size_t)hp->pitch * hp->rows % MCW_LINE == 0 && hp->base % MCW_LINE == 0, "plane %d is not whole lines", pl);
        // containment: the load stays in its row, and holds every column the interpolation reads
        CHECK(hw.ax >= 0 && hw.ax % 4 == 0 && hw.ax + v.len <= v.width, "load leaves the row: ax %d", hw.ax);
        for (int i = 0; i < v.n; i++) {
            const int x = clampi(v.x0 + i, 0, v.width - 1);
            CHECK(x >= hw.ax && x < hw.ax + v.len, "column %d outside [%d, %d)", x, hw.ax, hw.ax + v.len);
        }
        n_clamped += v.x0 < 0 || v.x0 + v.n > v.width || v.y0 < 0 || v.y0 + v.n > v.rows;
        // lines: every access, and the spans dep_wait_cols takes
        std::vector<Cells> acc(v.n);
        for (int k = 0; k < v.n; k++) {
            const int y = clampi(v.y0 + k, 0, v.rows - 1);
            CHECK(mcw_row(hp, hw.y0 + k) == y, "row %d", k);
            const size_t o = s.at(pl, v.ax, y);
            CHECK(o + v.len <= s.bytes && o + v.len <= s.at(pl, 0, 0) + (size_t)hp->pitch * hp->rows, "load leaves the plane");
            acc[k] = s.cells_of(o, v.len);
            const mcw_cells hc = mcw_access_cells(hp, hw.ax, v.len, y);
            n_accesses++;
            n_two_rows += s.line_rows2[o / 128] || s.line_rows2[(o + v.len - 1) / 128];
            CHECK(hc.r_lo == acc[k].r_lo && hc.r_hi == acc[k].r_hi && hc.x == acc[k].x,
                  "cells %dx%d plane %d x %d y %d: header %d..%d x %d, bytes %d..%d x %d", s.w, s.h, pl, v.ax, y, hc.r_lo, hc.r_hi,
                  hc.x, acc[k].r_lo, acc[k].r_hi, acc[k].x);
        }
        for (int first = 0; first < (pl == 0 ? 4 : 1); first++) {
            Cells u = acc[first];
            for (int k = first; k < v.n; k++) merge(u, acc[k]);
            const int ya = clampi(v.y0 + first, 0, v.rows - 1), yb = clampi(v.y0 + v.n - 1, 0, v.rows - 1);
            const mcw_cells hs = mcw_span_cells(hp, hw.ax, v.len, ya, yb);
            CHECK(hs.r_lo == u.r_lo && hs.r_hi == u.r_hi, "span rows: header %d..%d, bytes %d..%d", hs.r_lo, hs.r_hi, u.r_lo, u.r_hi);
            CHECK(hp->pitch % 128 == 0 ? hs.x == u.x : hs.x >= u.x && hs.x == s.w - 1, "span column %dx%d plane %d: header %d, bytes %d", s.w, s.h, pl, hs.x, u.x);
            const Cells k = dep_wait_cols_rule(s.w, s.h, pl != 0, mbx, mby, b, mvx, mvy, first);
            CHECK(k.r_lo == hs.r_lo && k.r_hi == hs.r_hi && k.x == hs.x, "dep_wait_cols' lines %dx%d plane %d: %d..%d x %d, header %d..%d x %d",
                  s.w, s.h, pl, k.r_lo, k.r_hi, k.x, hs.r_lo, hs.r_hi, hs.x);
        }
    }
}

// the lane map: 64 lanes load every row of every window, and the rows a
// lane is held to in the waits contain the rows it loads
static void check_lanes()
{
    std::set<std::pair<int, int>> luma;
    std::set<std::pair<int, int>> chroma;
    for (int lane = 0; lane < MCW_LANES; lane++) {
        for (int k = 0; k < MCW_LANE_LUMA_LOADS; k++) {
            const int row = mcw_lane_luma_row(lane, k);
            CHECK(row >= mcw_lane_luma_first(lane) && row < MCW_LUMA_ROWS, "lane %d luma row %d", lane, row);
            luma.insert({mcw_lane_luma_blk(lane), row});
        }
        for (int k = 0; k < MCW_LANE_CHROMA_LOADS; k++) {
            const int row = mcw_lane_chroma_row(lane, k);
            CHECK(row >= 0 && row < MCW_CHROMA_ROWS, "lane %d chroma row %d", lane, row);
            chroma.insert({mcw_lane_chroma_blk(lane) * 2 + mcw_lane_chroma_comp(lane), row});
        }
        CHECK(mcw_lane_luma_blk(lane) >= 0 && mcw_lane_luma_blk(lane) < 16 && mcw_lane_chroma_blk(lane) >= 0 &&
              mcw_lane_chroma_blk(lane) < 16 && (mcw_lane_chroma_comp(lane) | 1) == 1, "lane %d", lane);
    }
    CHECK(luma.size() == 16 * MCW_LUMA_ROWS, "luma (block, row) pairs loaded: %zu", luma.size());
    CHECK(chroma.size() == 32 * MCW_CHROMA_ROWS, "chroma (block, component, row) triples loaded: %zu", chroma.size());
    for (int b = 0; b < 16; b++)
        CHECK(mcw_blk_x(b) == BX[b] && mcw_blk_y(b) == BY[b] && mcw_blk_part(b) == b / 4, "block %d", b);
}

// the host's encodings from random inter records
static uint32_t g_rng = 12345;
static int rnd(int n) { g_rng = g_rng * 1664525u + 1013904223u; return (int)((g_rng >> 8) % (uint32_t)n); }
static long long n_records = 0;

static void check_records(const Slot &s)
{
    const size_t lines = s.bytes / 128;
    std::set<std::pair<int, size_t>> touched;                 // (slot, line) of every touched byte
    std::vector<uint8_t> mark(4 * lines, 0);                    // the header-based count (host/capture.c ref_line_bytes)
    size_t marked = 0;
    for (int mb = 0; mb < s.w * s.h; mb++) {
        MbRec r;
        std::memset(&r, 0, sizeof(r));
        r.type = rnd(2) ? MBT_INTER : MBT_SKIP;
        for (int q = 0; q < 4; q++) r.ref[q] = (uint8_t)rnd(4);
        const int far = rnd(4) == 0;
        for (int b = 0; b < 16; b++) {
            r.mv[b][0] = (int16_t)(far ? rnd(8 * (s.W16 + 40)) - 4 * (s.W16 + 40) : rnd(161) - 80);
            r.mv[b][1] = (int16_t)(far ? rnd(8 * (s.H16 + 40)) - 4 * (s.H16 + 40) : rnd(161) - 80);
        }
        const int mbx = mb % s.w, mby = mb / s.w;
        int want[4] = {0, 0, 0, 0};
        for (int b = 0; b < 16; b++)
            for (int pl = 0; pl < 3; pl++) {
                const Win v = window(s, pl, mbx, mby, b, r.mv[b][0], r.mv[b][1]);
                for (int k = 0; k < v.n; k++) {
                    const size_t o = s.at(pl, v.ax, clampi(v.y0 + k, 0, v.rows - 1));
                    want[b / 4] = std::max(want[b / 4], s.cells_of(o, v.len).r_hi);
                    for (int i = 0; i < v.len; i++) touched.insert({r.ref[b / 4], (o + i) / 128});
                }
            }
        uint16_t rows[4];
        mcw_ref_rows(&r, s.w, s.h, mbx, mby, rows);
        for (int q = 0; q < 4; q++)
            CHECK(rows[q] == want[q], "i4 %dx%d mb %d partition %d: header %d, bytes %d", s.w, s.h, mb, q, rows[q], want[q]);
        for (int b = 0; b < 16; b++) {
            uint32_t off[MCW_BLK_ACCESSES];
            mcw_blk_accesses(&r, s.w, s.h, mbx, mby, b, off);
            for (int j = 0; j < MCW_BLK_ACCESSES; j++)
                for (size_t l = off[j] / MCW_LINE; l <= (off[j] + mcw_blk_access_len(j) - 1) / MCW_LINE; l++) {
                    CHECK(l < lines, "line %zu outside the slot", l);
                    if (l < lines && !mark[r.ref[b / 4] * lines + l]) { mark[r.ref[b / 4] * lines + l] = 1; marked++; }
                }
        }
        n_records++;
    }
    CHECK(marked == touched.size(), "lines %dx%d: header %zu, bytes %zu", s.w, s.h, marked, touched.size());
}

int main()
{
    check_lanes();
    for (const auto &sz : SIZES) {
        const Slot s(sz[0], sz[1]);
        CHECK(s.bytes == H264MI_SLOT_BYTES(s.w, s.h) && s.CP == H264MI_CPITCH(s.w), "slot %dx%d", s.w, s.h);
        std::set<std::pair<int, int>> mbs;
        for (int x : {0, s.w / 2, s.w - 1})
            for (int y : {0, s.h / 2, s.h - 1}) mbs.insert({x, y});
        const std::vector<int> mx = mv_axis(s.W16), my = mv_axis(s.H16);
        for (const auto &mb : mbs)
            for (int b = 0; b < 16; b++)
                for (int mvx : mx)
                    for (int mvy : my) check_window(s, mb.first, mb.second, b, mvx, mvy);
        for (int rep = 0; rep < (s.w * s.h < 64 ? 8 : 2); rep++) check_records(s);
    }
    std::printf("%lld windows (%lld leave the picture), %lld accesses (%lld on lines of two sample rows), %lld records\n", n_windows,
                n_clamped, n_accesses, n_two_rows, n_records);
    if (g_bad || !n_clamped || !n_two_rows) { std::printf("FAILED: %lld mismatches\n", g_bad); return 1; }
    std::printf("ok %d sizes, %lld windows, %lld accesses, %lld records, 0 mismatches\n", (int)(sizeof(SIZES) / sizeof(SIZES[0])),
                n_windows, n_accesses, n_records);
    return 0;
}
