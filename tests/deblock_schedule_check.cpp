// The two-step deblocking pass of recon_kernels.hip deblock_dir on the CPU,
// driven by its lane map (broadway_amd/csrc/hip/deblock_lanes.h), against the
// standard's edge order.
//
// edge_ref() is a plain restatement of 8.7.2.3 / 8.7.2.4 for one edge of one
// line.  The reference runs it over the edges of a line one after another
// (edge 0, 1, 2, 3; chroma 0, 1).  The schedule runs a 64-lane wave on the
// lines of one MB as the kernel does: every lane loads what the map says,
// step A filters the MB edges and stores, step B filters every internal edge
// at once -- each lane computes its q1 first, the lane the map names takes it
// as its p2, the lanes of edge 1 take p2..p0 from what they held after step
// A -- and stores.  Both must leave the same samples, for every combination
// of bS (edge 0: 0..4, edges 1..3: 0..3, chroma: its two edges), with the
// (alpha, beta, tc0) of indexA / indexB 0..51 from common/tables.c, on
// pseudo-random lines of several spreads, flat lines and step lines, in both
// directions (rows stored in dwords and 16-bit halves, columns in bytes).
//
// From the header alone, per step and direction, it also proves that no
// sample has two owners or is stored by two lanes, that every sample the
// sequential filter can change has an owner, and that no lane's filter reads
// a sample a lane of an earlier edge owns in the same step, other than the
// one p2 hand-over.  (A later edge's p1 is an earlier edge's q2: it is read
// at the value it had before the step, as in the standard's order, because
// every load of a pass precedes its stores.)
//
// Prints "ok ..." at the end; a mismatch is reported on stderr and fails the
// run.  tests/test_deblock_schedule.py builds this with AddressSanitizer +
// UBSan.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../broadway_amd/csrc/hip/deblock_lanes.h"
extern "C" {
#include "../broadway_amd/csrc/common/tables.h"
}

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, " [%s]\n", #cond); } } } while (0)

struct Thr { int alpha, beta, tc0[3]; };

static int iabs(int x) { return x < 0 ? -x : x; }
static int clip3(int lo, int hi, int x) { return x < lo ? lo : x > hi ? hi : x; }
static int clip1(int x) { return clip3(0, 255, x); }

// one edge of one line, s = p3 p2 p1 p0 q0 q1 q2 q3 (chroma uses p1..q1)
static void edge_ref(int *s, int bS, const Thr &t, bool chroma)
{
    const int p3 = s[0], p2 = s[1], p1 = s[2], p0 = s[3], q0 = s[4], q1 = s[5], q2 = s[6], q3 = s[7];
    if (bS == 0) return;
    if (!(iabs(p0 - q0) < t.alpha && iabs(p1 - p0) < t.beta && iabs(q1 - q0) < t.beta)) return;
    if (bS < 4) {
        const int tc0 = t.tc0[bS - 1];
        const bool ap = !chroma && iabs(p2 - p0) < t.beta, aq = !chroma && iabs(q2 - q0) < t.beta;
        const int tc = chroma ? tc0 + 1 : tc0 + (ap ? 1 : 0) + (aq ? 1 : 0);
        const int delta = clip3(-tc, tc, (((q0 - p0) * 4) + (p1 - q1) + 4) >> 3);
        s[3] = clip1(p0 + delta);
        s[4] = clip1(q0 - delta);
        if (ap) s[2] = p1 + clip3(-tc0, tc0, (p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1);
        if (aq) s[5] = q1 + clip3(-tc0, tc0, (q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1);
        return;
    }
    const bool small = iabs(p0 - q0) < (t.alpha >> 2) + 2;
    if (!chroma && iabs(p2 - p0) < t.beta && small) {
        s[3] = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3;
        s[2] = (p2 + p1 + p0 + q0 + 2) >> 2;
        s[1] = (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3;
    } else {
        s[3] = (2 * p1 + p0 + q1 + 2) >> 2;
    }
    if (!chroma && iabs(q2 - q0) < t.beta && small) {
        s[4] = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3;
        s[5] = (p0 + q0 + q1 + q2 + 2) >> 2;
        s[6] = (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3;
    } else {
        s[4] = (2 * q1 + q0 + p1 + 2) >> 2;
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

// one MB's lines of one direction: 16 luma lines of 20 samples, 8 + 8 chroma
// lines of 12 (kept in 20), their bS per edge and the four threshold classes
enum { NLINES = DBL_LUMA_LINES + 2 * DBL_CHROMA_LINES };
struct Mb {
    int s[NLINES][DBL_LUMA_SAMPLES];
    int bS[NLINES][4];          // by luma edge: a chroma line's edges 0, 1 are nibbles 0, 2
    Thr thr[2][2];              // [chroma][internal]
};
static int line_of(int plane, int line) { return plane == DBL_LUMA ? line : DBL_LUMA_LINES + (plane - 1) * DBL_CHROMA_LINES + line; }

static Thr thr_of(int ia, int ib)
{
    Thr t;
    t.alpha = kAlpha[ia]; t.beta = kBeta[ib];
    for (int i = 0; i < 3; i++) t.tc0[i] = kTc0[ia][i];
    return t;
}

static void reference(Mb &m)
{
    for (int l = 0; l < NLINES; l++) {
        const bool chroma = l >= DBL_LUMA_LINES;
        for (int k = 0; k < (chroma ? 2 : 4); k++)
            edge_ref(&m.s[l][4 * k], m.bS[l][chroma ? 2 * k : k], m.thr[chroma][k > 0], chroma);
    }
}

// the wave; skipped[step] counts the steps no lane had a bS for
static void schedule(Mb &m, int dir, long *skipped)
{
    int rega[DBL_LANES][8];
    for (int step = DBL_STEP_A; step <= DBL_STEP_B; step++) {
        int reg[DBL_LANES][8], bs[DBL_LANES], q1res[DBL_LANES];
        bool any = false;
        // loads: all of them before any store of the step
        for (int lane = 0; lane < DBL_LANES; lane++) {
            const int l = line_of(dbl_plane(lane), dbl_line(lane)), k = dbl_edge(step, lane);
            memset(reg[lane], 0, sizeof(reg[lane]));
            const int lf = dbl_load_first(step, k), e0 = 4 * k;
            for (int i = 0; i < dbl_load_count(step); i++) reg[lane][lf + i - e0] = m.s[l][lf + i];
            bs[lane] = m.bS[l][dbl_bs_nibble(step, lane)];
            any = any || bs[lane] != 0;
            if (step == DBL_STEP_B && dbl_b_from_a(lane))
                for (int i = 1; i <= 3; i++) reg[lane][i] = rega[lane][4 + i];     // samples 5..7, as the lane held them after step A
        }
        if (!any) skipped[step]++;
        if (!any && step == DBL_STEP_B) return;        // (step A stores what it loaded when skipped)
        // step B: every lane's q1 first -- it must not depend on the lane's p2
        if (step == DBL_STEP_B)
            for (int lane = 0; lane < DBL_LANES; lane++) {
                const bool chroma = dbl_chroma(lane);
                int lo[8], hi[8];
                memcpy(lo, reg[lane], sizeof(lo)); memcpy(hi, reg[lane], sizeof(hi));
                lo[1] = 0; hi[1] = 255;
                edge_ref(lo, bs[lane], m.thr[chroma][1], chroma);
                edge_ref(hi, bs[lane], m.thr[chroma][1], chroma);
                CHECK(lo[5] == hi[5], "lane %d: q1 depends on p2", lane);
                q1res[lane] = lo[5];
            }
        for (int lane = 0; lane < DBL_LANES; lane++) {
            const bool chroma = dbl_chroma(lane);
            if (step == DBL_STEP_B) {
                // the hand-over, as the kernel's quad_perm move makes it
                const int src = (lane & ~3) | ((DBL_P2_QUAD_PERM >> (2 * (lane & 3))) & 3);
                if (!dbl_b_from_a(lane)) {
                    CHECK(src == dbl_p2_from(lane), "lane %d: quad_perm source %d, map %d", lane, src, dbl_p2_from(lane));
                    reg[lane][1] = q1res[src];
                } else {
                    CHECK(dbl_p2_from(lane) == -1, "lane %d takes p2 from two places", lane);
                }
            }
            if (any) edge_ref(reg[lane], bs[lane], m.thr[chroma][step == DBL_STEP_B], chroma);
            if (step == DBL_STEP_B) CHECK(reg[lane][5] == q1res[lane], "lane %d: q1 changed after the hand-over", lane);
        }
        for (int lane = 0; lane < DBL_LANES; lane++) {
            if (!dbl_stores(step, lane)) continue;
            const bool chroma = dbl_chroma(lane);
            const int l = line_of(dbl_plane(lane), dbl_line(lane)), k = dbl_edge(step, lane);
            const int sf = dbl_store_first(dir, step, chroma, k);
            for (int i = 0; i < dbl_store_count(dir, step, chroma); i++) m.s[l][sf + i] = reg[lane][sf + i - 4 * k];
        }
        if (step == DBL_STEP_A) memcpy(rega, reg, sizeof(rega));
    }
}

// ---- the map's properties, from the header alone
static void prove_map()
{
    for (int dir = 0; dir < 2; dir++)
        for (int step = DBL_STEP_A; step <= DBL_STEP_B; step++) {
            int owner[NLINES][DBL_LUMA_SAMPLES], storer[NLINES][DBL_LUMA_SAMPLES], lane_of_edge[NLINES][4];
            memset(owner, -1, sizeof(owner)); memset(storer, -1, sizeof(storer)); memset(lane_of_edge, -1, sizeof(lane_of_edge));
            for (int lane = 0; lane < DBL_LANES; lane++) {
                const bool chroma = dbl_chroma(lane);
                const int plane = dbl_plane(lane), line = dbl_line(lane), k = dbl_edge(step, lane);
                const int nsamp = chroma ? DBL_CHROMA_SAMPLES : DBL_LUMA_SAMPLES;
                CHECK(plane >= DBL_LUMA && plane <= DBL_CR && line >= 0 && line < (chroma ? DBL_CHROMA_LINES : DBL_LUMA_LINES), "lane %d: line", lane);
                CHECK(k >= 0 && k < (chroma ? 2 : 4) && (k == 0) == (step == DBL_STEP_A), "lane %d: edge %d", lane, k);
                CHECK(dbl_bs_nibble(step, lane) == (chroma ? 2 * k : k), "lane %d: bS nibble", lane);
                CHECK(dbl_bs_seg(lane) == (chroma ? line >> 1 : line >> 2), "lane %d: bS segment", lane);
                const int l = line_of(plane, line);
                const int rf = dbl_read_first(step, chroma, k), rc = dbl_read_count(step, chroma);
                const int lf = dbl_load_first(step, k), lc = dbl_load_count(step);
                const int of = dbl_own_first(step, chroma, k), oc = dbl_own_count(step, chroma);
                const int sf = dbl_store_first(dir, step, chroma, k), sc = dbl_store_count(dir, step, chroma);
                CHECK(lf >= 0 && lf + lc <= DBL_LUMA_SAMPLES, "lane %d: loads outside the region", lane);
                CHECK(rf >= lf && rf + rc <= lf + lc && rf + rc <= nsamp, "lane %d: reads what it does not load", lane);
                CHECK(of >= sf && of + oc <= sf + sc, "lane %d: owns what it does not store", lane);
                CHECK(sf >= lf && sf + sc <= lf + lc && sf + sc <= nsamp, "lane %d: stores what it did not load", lane);
                // the edge's p's and q's as the filter sees them
                CHECK(rf == 4 * k + (chroma ? 2 : step == DBL_STEP_A ? 0 : 1), "lane %d: read window", lane);
                // rows: dwords in step A, aligned 16-bit halves in step B
                if (dir == 0) CHECK(step == DBL_STEP_A ? (sf % 4 == 0 && sc % 4 == 0) : (sf % 2 == 0 && sc % 2 == 0), "lane %d: row store alignment", lane);
                if (!dbl_stores(step, lane)) {
                    // a lane that stores nothing repeats a storing lane of its quad: same luma line, same edge
                    CHECK(!chroma && step == DBL_STEP_A, "lane %d stores nothing", lane);
                    continue;
                }
                CHECK(lane_of_edge[l][k] == -1, "line %d edge %d: lanes %d and %d", l, k, lane_of_edge[l][k], lane);
                lane_of_edge[l][k] = lane;
                for (int i = of; i < of + oc; i++) { CHECK(owner[l][i] == -1, "dir %d step %d line %d sample %d: owners %d and %d", dir, step, l, i, owner[l][i], lane); owner[l][i] = lane; }
                for (int i = sf; i < sf + sc; i++) { CHECK(storer[l][i] == -1, "dir %d step %d line %d sample %d: stored by %d and %d", dir, step, l, i, storer[l][i], lane); storer[l][i] = lane; }
            }
            // every sample the sequential filter can change in the step's edges has an owner
            for (int l = 0; l < NLINES; l++) {
                const bool chroma = l >= DBL_LUMA_LINES;
                for (int k = 0; k < (chroma ? 2 : 4); k++) {
                    if ((k == 0) != (step == DBL_STEP_A)) continue;
                    CHECK(lane_of_edge[l][k] >= 0, "step %d line %d edge %d: no lane", step, l, k);
                    const int cf = 4 * k + (chroma ? 3 : k == 0 ? 1 : 2), cc = chroma ? 2 : k == 0 ? 6 : 4;
                    for (int i = cf; i < cf + cc; i++) CHECK(owner[l][i] == lane_of_edge[l][k], "step %d line %d edge %d sample %d: owner %d", step, l, k, i, owner[l][i]);
                }
            }
            // reads against the owners of earlier edges of the step
            for (int lane = 0; lane < DBL_LANES; lane++) {
                const bool chroma = dbl_chroma(lane);
                const int l = line_of(dbl_plane(lane), dbl_line(lane)), k = dbl_edge(step, lane);
                const int rf = dbl_read_first(step, chroma, k), rc = dbl_read_count(step, chroma);
                int crossing = 0;
                for (int i = rf; i < rf + rc; i++) {
                    const int o = owner[l][i];
                    if (o < 0 || dbl_edge(step, o) >= k) continue;
                    crossing++;
                    CHECK(!chroma && i == 4 * k + 1 && o == dbl_p2_from(lane), "step %d lane %d reads sample %d of lane %d", step, lane, i, o);
                }
                CHECK(crossing == (dbl_p2_from(lane) >= 0 && step == DBL_STEP_B ? 1 : 0), "step %d lane %d: %d crossing reads", step, lane, crossing);
                if (step == DBL_STEP_B && dbl_p2_from(lane) >= 0) {
                    const int f = dbl_p2_from(lane);
                    CHECK(line_of(dbl_plane(f), dbl_line(f)) == l && dbl_edge(step, f) == k - 1 && (f >> 2) == (lane >> 2), "lane %d: p2 from lane %d", lane, f);
                }
                // what a lane of edge 1 keeps from step A is its own line's MB edge, computed by itself
                if (step == DBL_STEP_B && dbl_b_from_a(lane)) CHECK(k == 1 && dbl_edge(DBL_STEP_A, lane) == 0 && dbl_load_first(DBL_STEP_A, 0) + dbl_load_count(DBL_STEP_A) == 8, "lane %d: step A registers", lane);
                if (step == DBL_STEP_B && !dbl_b_from_a(lane)) CHECK(k >= 2 && dbl_load_first(step, k) > dbl_own_first(DBL_STEP_A, chroma, 0) + dbl_own_count(DBL_STEP_A, chroma) - 1, "lane %d loads what step A changes", lane);
            }
        }
}

static void fill_line(int *s, int n, int kind)
{
    static const int spread[] = {1, 2, 3, 5, 9, 17, 40, 256};
    if (kind == 8) {                    // all equal
        const int v = (int)(rnd() & 255);
        for (int i = 0; i < n; i++) s[i] = v;
    } else if (kind == 9) {             // a step somewhere, small noise on both levels
        const int a = (int)(rnd() & 255), b = (int)(rnd() & 255), at = (int)(rnd() % (unsigned)n), nz = (int)(rnd() & 3);
        for (int i = 0; i < n; i++) s[i] = clip1((i < at ? a : b) + (nz ? (int)(rnd() % (unsigned)(nz + 1)) : 0));
    } else if (kind == 10) {            // a ramp
        const int a = (int)(rnd() & 255), d = (int)(rnd() % 9) - 4;
        for (int i = 0; i < n; i++) s[i] = clip1(a + d * i + (int)(rnd() & 1));
    } else {
        const int sp = spread[kind], base = sp >= 256 ? 0 : (int)(rnd() % (unsigned)(257 - sp));
        for (int i = 0; i < n; i++) s[i] = base + (int)(rnd() % (unsigned)sp);
    }
}

int main()
{
    prove_map();
    if (failures) { fprintf(stderr, "%d failures in the lane map\n", failures); return 1; }
    const int NMB = 65536;              // x 16 lines: > 10^6 luma and 10^6 chroma lines per direction
    static long luma_combo[5 * 64], chroma_combo[5 * 4];
    long lines[2][2] = {{0, 0}, {0, 0}}, changed = 0, skipped[2][2] = {{0, 0}, {0, 0}}, ia_seen[52] = {0};
    for (int dir = 0; dir < 2; dir++)
        for (int n = 0; n < NMB; n++) {
            Mb m;
            memset(&m, 0, sizeof(m));
            for (int c = 0; c < 2; c++)
                for (int in = 0; in < 2; in++) {
                    // real index pairs: mostly close together (indexA and indexB differ by the slice offsets), some free
                    const int ia = (int)(rnd() % 52), ib = (rnd() & 3) ? clip3(0, 51, ia + (int)(rnd() % 13) - 6) : (int)(rnd() % 52);
                    m.thr[c][in] = thr_of(ia, ib);
                    ia_seen[ia]++;
                }
            const int forced = n & 7;   // 1: no MB edge anywhere (step A skipped), 2: no internal edge (step B skipped), 3: neither
            for (int l = 0; l < NLINES; l++) {
                const bool chroma = l >= DBL_LUMA_LINES;
                const long id = (long)n * 16 + (chroma ? l - DBL_LUMA_LINES : l);
                if (!chroma) {
                    const int combo = (int)((id + dir * 7) % (5 * 64));
                    m.bS[l][0] = combo >> 6; m.bS[l][1] = combo & 3; m.bS[l][2] = (combo >> 2) & 3; m.bS[l][3] = (combo >> 4) & 3;
                } else {
                    const int combo = (int)((id + dir * 3) % (5 * 4));
                    m.bS[l][0] = combo >> 2; m.bS[l][2] = combo & 3;
                }
                if (forced == 1 || forced == 3) m.bS[l][0] = 0;
                if (forced == 2 || forced == 3) m.bS[l][1] = m.bS[l][2] = m.bS[l][3] = 0;
                if (!chroma) luma_combo[(m.bS[l][0] << 6) | m.bS[l][1] | (m.bS[l][2] << 2) | (m.bS[l][3] << 4)]++;
                else chroma_combo[(m.bS[l][0] << 2) | m.bS[l][2]]++;
                fill_line(m.s[l], chroma ? DBL_CHROMA_SAMPLES : DBL_LUMA_SAMPLES, (int)(rnd() % 11));
                lines[dir][chroma]++;
            }
            Mb ref = m, got = m;
            reference(ref);
            schedule(got, dir, skipped[dir]);
            for (int l = 0; l < NLINES; l++) {
                if (memcmp(ref.s[l], m.s[l], sizeof(m.s[l]))) changed++;
                if (memcmp(ref.s[l], got.s[l], sizeof(ref.s[l]))) {
                    CHECK(false, "dir %d MB %d line %d (bS %d %d %d %d): the schedule differs from the edge order", dir, n, l,
                          m.bS[l][0], m.bS[l][1], m.bS[l][2], m.bS[l][3]);
                }
            }
        }
    for (int i = 0; i < 5 * 64; i++) CHECK(luma_combo[i] > 100, "luma bS combination %d: %ld lines", i, luma_combo[i]);
    for (int i = 0; i < 5 * 4; i++) CHECK(chroma_combo[i] > 100, "chroma bS combination %d: %ld lines", i, chroma_combo[i]);
    for (int i = 0; i < 52; i++) CHECK(ia_seen[i] > 100, "indexA %d: %ld classes", i, ia_seen[i]);
    for (int dir = 0; dir < 2; dir++) {
        CHECK(lines[dir][0] >= 1000000 && lines[dir][1] >= 1000000, "dir %d: %ld luma, %ld chroma lines", dir, lines[dir][0], lines[dir][1]);
        CHECK(skipped[dir][0] > 1000 && skipped[dir][1] > 1000, "dir %d: steps skipped %ld, %ld times", dir, skipped[dir][0], skipped[dir][1]);
    }
    // the lines are not all left alone by the filter
    CHECK(changed > (lines[0][0] + lines[0][1]) / 10, "only %ld lines changed", changed);
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("lines per direction: %ld luma %ld chroma; %ld of all lines changed by the filter\n", lines[0][0], lines[0][1], changed);
    printf("ok %d luma %d chroma bS combinations, 2 directions, 0 mismatches\n", 5 * 64, 5 * 4);
    return 0;
}
