// The lane map of one deblocking pass (recon_kernels.hip deblock_dir), stated
// once.  Plain C++17, no HIP: the kernel takes its lines, edges, offsets and
// the cross-lane move from here, and tests/deblock_schedule_check.cpp runs the
// same map on the CPU against the standard's edge order.
//
// A line is one row (dir 0, vertical edges) or one column (dir 1, horizontal
// edges) of the MB with its 4-sample halo: samples 0..19 are positions
// -4..15 across the edges, edge k lies between samples 4k+3 and 4k+4, so
// p3..q3 of edge k are samples 4k..4k+7.  A chroma line has samples 0..11
// and its two edges sit where luma edges 0 and 1 do.
//
// A pass is two steps on one wave:
//   step A  the MB edge (edge 0, the only one that can carry bS 4) of all
//           32 lines;
//   step B  every internal edge at once: 16 luma lines x edges 1..3 and 16
//           chroma lines x chroma edge 1 = 64 lanes.
// With bS < 4 an edge changes p1..q1 only and takes from the edge before it
// one sample, its p2 (that edge's q1), whose new value does not depend on
// that edge's own p2.  So each step B lane computes its q1, hands it to the
// lane of the next edge, and finishes.
//
// Lane = 4 * q + e.  The four lanes of quad q work on luma line q (e = 1..3)
// and on chroma line q (e = 0: Cb lines 0..7 in quads 0..7, Cr in 8..15):
//   step A  e = 0 the chroma line's MB edge, e = 1 the luma line's; e = 2, 3
//           compute what e = 1 computes and store nothing;
//   step B  e = 0 the chroma line's edge 1, e = 1..3 the luma line's edge e.
// So the p2 hand-over is a move by one lane inside a quad (one DPP quad_perm),
// and the lane of luma edge 1 (and of chroma edge 1) is the lane that ran the
// same line's MB edge: what step A left it takes from its own registers.
#ifndef H264MI_DEBLOCK_LANES_H
#define H264MI_DEBLOCK_LANES_H

enum { DBL_LUMA = 0, DBL_CB = 1, DBL_CR = 2 };
enum { DBL_STEP_A = 0, DBL_STEP_B = 1 };
enum { DBL_LANES = 64, DBL_LUMA_LINES = 16, DBL_CHROMA_LINES = 8, DBL_LUMA_SAMPLES = 20, DBL_CHROMA_SAMPLES = 12 };

// the lane's line: the same one in both steps and both directions
constexpr bool dbl_chroma(int lane) { return (lane & 3) == 0; }
constexpr int dbl_plane(int lane) { return !dbl_chroma(lane) ? DBL_LUMA : (lane >> 2) >= DBL_CHROMA_LINES ? DBL_CR : DBL_CB; }
constexpr int dbl_line(int lane) { return dbl_chroma(lane) ? (lane >> 2) & (DBL_CHROMA_LINES - 1) : lane >> 2; }
// its edge in a step (a chroma line's edge 1 is the picture's luma edge 2: dbl_bs_nibble)
constexpr int dbl_edge(int step, int lane) { return step == DBL_STEP_A ? 0 : dbl_chroma(lane) ? 1 : lane & 3; }
// whether the lane stores in the step (step A's lanes e = 2, 3 repeat lane e = 1)
constexpr bool dbl_stores(int step, int lane) { return step == DBL_STEP_B || (lane & 3) < 2; }
// the nibble of the line's 16-bit bS word (one nibble per luma edge) that holds the lane's bS
constexpr int dbl_bs_nibble(int step, int lane) { return step == DBL_STEP_A ? 0 : dbl_chroma(lane) ? 2 : lane & 3; }
// the 4-line segment of the MB edge the line's bS word belongs to
constexpr int dbl_bs_seg(int lane) { return dbl_chroma(lane) ? dbl_line(lane) >> 1 : dbl_line(lane) >> 2; }

// Samples of the line the filter of (step, plane, edge) reads: p3..q3 at the
// MB edge, p2..q2 at an internal edge, p1..q1 for chroma.
constexpr int dbl_read_first(int step, bool chroma, int edge) { return 4 * edge + (chroma ? 2 : step == DBL_STEP_A ? 0 : 1); }
constexpr int dbl_read_count(int step, bool chroma) { return chroma ? 4 : step == DBL_STEP_A ? 8 : 6; }
// Samples the lane loads: the luma set for every lane (a chroma lane uses
// p1..q1 of it; in a column's step A the first two lie above the plane and
// are neither used nor stored).  Every load of a pass precedes its stores.
constexpr int dbl_load_first(int step, int edge) { return dbl_read_first(step, false, edge); }
constexpr int dbl_load_count(int step) { return dbl_read_count(step, false); }
// Samples the filter can change, which the lane owns in the step: p2..q2 at
// the MB edge, p1..q1 inside, p0 and q0 for chroma.
constexpr int dbl_own_first(int step, bool chroma, int edge) { return 4 * edge + (chroma ? 3 : step == DBL_STEP_A ? 1 : 2); }
constexpr int dbl_own_count(int step, bool chroma) { return chroma ? 2 : step == DBL_STEP_A ? 6 : 4; }
// Samples the lane stores.  Rows (dir 0) are stored in dwords in step A --
// the halo dword and dword 1 of the line, p3..q3 -- and in 16-bit halves in
// step B; columns (dir 1) byte by byte, exactly what is owned in step A.  A
// step B lane stores p1..q1 in both directions, a chroma lane too: its p1 and
// q1 go back as they were read (no other lane touches the line in the step).
constexpr int dbl_store_first(int dir, int step, bool chroma, int edge)
{
    return step == DBL_STEP_B ? 4 * edge + 2 : dir == 0 ? 0 : dbl_own_first(step, chroma, edge);
}
constexpr int dbl_store_count(int dir, int step, bool chroma)
{
    return step == DBL_STEP_B ? 4 : dir == 0 ? 8 : dbl_own_count(step, chroma);
}

// Step B: the lane whose q1 result is this lane's p2, -1: none (edge 1 and
// chroma read the sample the MB edge left).  The kernel makes the move with
// one DPP quad_perm, DBL_P2_QUAD_PERM: lane e of a quad takes from lane
// max(e - 1, 0).
constexpr int dbl_p2_from(int lane) { return (lane & 3) >= 2 ? lane - 1 : -1; }
constexpr int dbl_quad_src(int e) { return e > 0 ? e - 1 : 0; }
constexpr int DBL_P2_QUAD_PERM = dbl_quad_src(0) | (dbl_quad_src(1) << 2) | (dbl_quad_src(2) << 4) | (dbl_quad_src(3) << 6);
// Step B lanes that take p2, p1 and p0 from what the same lane held after
// step A (samples 5..7 of the line): those of edge 1
constexpr bool dbl_b_from_a(int lane) { return dbl_edge(DBL_STEP_B, lane) == 1; }

static_assert(DBL_P2_QUAD_PERM == 0x90, "quad_perm [0, 0, 1, 2]");
static_assert(dbl_plane(0) == DBL_CB && dbl_plane(32) == DBL_CR && dbl_plane(33) == DBL_LUMA && dbl_line(33) == 8, "");
static_assert(dbl_read_first(DBL_STEP_B, false, 3) + dbl_read_count(DBL_STEP_B, false) <= DBL_LUMA_SAMPLES, "");
static_assert(dbl_read_first(DBL_STEP_B, true, 1) + dbl_read_count(DBL_STEP_B, true) <= DBL_CHROMA_SAMPLES, "");

#endif
