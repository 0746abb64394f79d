/* warp_taps (broadway_amd/csrc/common/warp_geom.h), where the affine-warped
 * export samples its window, proven on the CPU before the kernel sees an
 * extreme matrix: for every matrix the function names no position outside the
 * window.  Three parts:
 *   sweep    every matrix with coefficients in {0, +-1, +-65535, +-65536,
 *            +-2^24, INT32_MIN, INT32_MAX} (11^6), on the windows 2x2 and
 *            48x32, both borders, at three outputs;
 *   random   generated matrices over every even window 2x2 .. 48x32, both
 *            borders, any output of 16384 x 16384 -- each against a restatement
 *            in wide integers written from the definition of include/h264mi.h,
 *            and each tile warp_tile_outside calls outside checked output by
 *            output;
 *   digest   FNV-1a over the taps of 4096 generated cases, which
 *            tests/_warp.py reproduces in Python integers.
 * Lines: "sweep <matrices> <taps> ok", "random <cases> tiles_outside <n> ok",
 * "digest <hex>".  Built with AddressSanitizer + UBSan (shift excluded: the
 * arithmetic right shifts of negative positions are the definition). */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include "../broadway_amd/csrc/common/warp_geom.h"

static const int kSpecial[11] = {0, 1, -1, 65535, -65535, 65536, -65536, 1 << 24, -(1 << 24), INT_MIN, INT_MAX};

static unsigned long long g_taps;

static void fail(const char *what, const int *m, int i, int j, int cw, int ch, int border)
{
    printf("FAIL %s m %d %d %d %d %d %d i %d j %d window %dx%d border %d\n", what, m[0], m[1], m[2], m[3], m[4], m[5], i,
           j, cw, ch, border);
    exit(1);
}

/* what every caller relies on: positions inside the window, fractions in 0..255, a 4-bit mask */
static warp_tap checked(const int *m, int i, int j, int cw, int ch, int border)
{
    const warp_tap t = warp_taps(m, i, j, cw, ch, border);
    if (t.x[0] < 0 || t.x[0] >= cw || t.x[1] < 0 || t.x[1] >= cw || t.y[0] < 0 || t.y[0] >= ch || t.y[1] < 0 ||
        t.y[1] >= ch)
        fail("position outside the window", m, i, j, cw, ch, border);
    if (t.fx < 0 || t.fx > 255 || t.fy < 0 || t.fy > 255 || (t.mask & ~15) ||
        (border == H264MI_WARP_BORDER_REPLICATE && t.mask != 15))
        fail("fraction or mask", m, i, j, cw, ch, border);
    g_taps++;
    return t;
}

/* floor(a / 2^s) of a wide integer, by division (no shift of a negative value) */
static __int128 floor_shift(__int128 a, int s)
{
    const __int128 d = (__int128)1 << s, q = a / d;
    return a % d < 0 ? q - 1 : q;
}

/* the definition, unsaturated, in 128-bit integers: tap 2 dy + dx is real iff it lies in the window, and then (or
 * with REPLICATE, clamped) it is the position named */
static void against_definition(const int *m, int i, int j, int cw, int ch, int border)
{
    const warp_tap t = checked(m, i, j, cw, ch, border);
    const __int128 X = (__int128)m[0] * j + (__int128)m[1] * i + m[2], Y = (__int128)m[3] * j + (__int128)m[4] * i + m[5];
    const __int128 Xr = floor_shift(X + 128, 8), Yr = floor_shift(Y + 128, 8);
    const __int128 x0 = floor_shift(Xr, 8), y0 = floor_shift(Yr, 8);
    if (t.fx != (int)(Xr - x0 * 256) || t.fy != (int)(Yr - y0 * 256)) fail("fraction", m, i, j, cw, ch, border);
    for (int k = 0; k < 4; k++) {
        const __int128 x = x0 + (k & 1), y = y0 + (k >> 1);
        const int in = x >= 0 && x < cw && y >= 0 && y < ch;
        const __int128 cx = x < 0 ? 0 : x > cw - 1 ? cw - 1 : x, cy = y < 0 ? 0 : y > ch - 1 ? ch - 1 : y;
        if (border == H264MI_WARP_BORDER_CONSTANT && ((t.mask >> k) & 1) != in) fail("mask", m, i, j, cw, ch, border);
        if ((in || border == H264MI_WARP_BORDER_REPLICATE) && (t.x[k & 1] != (int)cx || t.y[k >> 1] != (int)cy))
            fail("tap", m, i, j, cw, ch, border);
    }
}

/* xorshift64* (Vigna); tests/_warp.py's Rng */
static uint64_t g_rng;
static uint32_t rnd(void)
{
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545F4914F6CDD1DULL) >> 32);
}

static int rnd_coef(void)
{
    const uint32_t kind = rnd() % 3, v = rnd();
    if (kind == 0) return kSpecial[v % 11];
    if (kind == 1) return (int)(int64_t)(v >= 0x80000000u ? (int64_t)v - ((int64_t)1 << 32) : (int64_t)v);
    return (int)(v % (1u << 19)) - (1 << 18);
}

int main(void)
{
    /* sweep */
    static const int win[2][2] = {{2, 2}, {48, 32}}, at[3][2] = {{0, 0}, {7, 31}, {16383, 16383}};
    unsigned long long mats = 0;
    int idx[6] = {0, 0, 0, 0, 0, 0};
    for (;;) {
        int m[6];
        for (int k = 0; k < 6; k++) m[k] = kSpecial[idx[k]];
        for (int w = 0; w < 2; w++)
            for (int b = 0; b < 2; b++)
                for (int p = 0; p < 3; p++) checked(m, at[p][0], at[p][1], win[w][0], win[w][1], b);
        mats++;
        int k = 0;
        while (k < 6 && ++idx[k] == 11) idx[k++] = 0;
        if (k == 6) break;
    }
    printf("sweep %llu %llu ok\n", mats, g_taps);

    /* random: every even window 2x2 .. 48x32 in turn */
    g_rng = 0xD1B54A32D192ED03ULL;
    unsigned long long cases = 0, outside = 0;
    for (int round = 0; round < 64; round++)
        for (int cw = 2; cw <= 48; cw += 2)
            for (int ch = 2; ch <= 32; ch += 2) {
                int m[6];
                for (int k = 0; k < 6; k++) m[k] = rnd_coef();
                const int border = (int)(rnd() & 1), i = (int)(rnd() % 16384), j = (int)(rnd() % 16384);
                against_definition(m, i, j, cw, ch, border);
                against_definition(m, 0, 0, cw, ch, border);
                cases += 2;
                /* the 32 x 8 tile that holds (i, j) */
                const int i0 = i & ~7, j0 = j & ~31;
                if (!warp_tile_outside(m, i0, i0 + 7, j0, j0 + 31, cw, ch)) continue;
                outside++;
                for (int di = 0; di < 8; di++)
                    for (int dj = 0; dj < 32; dj++)
                        if (checked(m, i0 + di, j0 + dj, cw, ch, H264MI_WARP_BORDER_CONSTANT).mask)
                            fail("a tile called outside holds a sample", m, i0 + di, j0 + dj, cw, ch, 0);
            }
    printf("random %llu tiles_outside %llu ok\n", cases, outside);

    /* digest */
    g_rng = 0x9E3779B97F4A7C15ULL;
    uint64_t h = 0xCBF29CE484222325ULL;
    for (int c = 0; c < 4096; c++) {
        int m[6];
        for (int k = 0; k < 6; k++) m[k] = rnd_coef();
        const int cw = 2 + 2 * (int)(rnd() % 24), ch = 2 + 2 * (int)(rnd() % 16);
        const int border = (int)(rnd() & 1);
        const int i = (int)(rnd() % 16384), j = (int)(rnd() % 16384);
        const warp_tap t = checked(m, i, j, cw, ch, border);
        const int v[7] = {t.fx, t.fy, t.x[0], t.x[1], t.y[0], t.y[1], t.mask};
        for (int k = 0; k < 7; k++)
            for (int b = 0; b < 4; b++) h = (h ^ (((uint32_t)v[k] >> (8 * b)) & 255u)) * 0x100000001B3ULL;
    }
    printf("digest %016llx\n", (unsigned long long)h);
    return 0;
}
