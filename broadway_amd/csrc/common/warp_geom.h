/* Where an affine-warped export (include/h264mi.h) samples its
 * window, stated once.  Plain C11 / C++17, no HIP: the kernel (hip/warp.hip)
 * takes every tap from warp_taps, tests/warp_geom_check.c proves over extreme
 * matrices that no tap leaves the window, and tests/_warp.py restates the
 * arithmetic in Python integers against the same program's digest.
 *
 * Output (row i, column j) of a warp with the Q16 coefficients m[0..5] sits at
 *   X = m0 j + m1 i + m2,  Y = m3 j + m4 i + m5      (exact: |X| < 2^47)
 * in the window, sample (c, r) being (c << 16, r << 16).  Per axis
 *   Pr = (P + 128) >> 8   (arithmetic: floor), p0 = Pr >> 8, f = Pr & 255:
 * the taps are p0 and p0 + 1 with weights 256 - f and f.  p0 is saturated to
 * [-2, n]: at -2 and below both taps lie in front of the window, at n and
 * above both lie behind it, and that is all a far-away position has to say --
 * so everything behind the 64-bit position fits an int.  A tap position is
 * always clamped into [0, n): it is the sample H264MI_WARP_BORDER_REPLICATE
 * takes, and with H264MI_WARP_BORDER_CONSTANT a tap outside the window is not
 * in the mask and counts as the pad sample, but what is named is in the window
 * still, so a caller may load every named position without a branch. */
#ifndef H264MI_WARP_GEOM_H
#define H264MI_WARP_GEOM_H

#include <stdint.h>
#include "../../../include/h264mi.h"

/* always_inline, like the kernel's own __forceinline__ helpers */
#ifdef __cplusplus
#define WARP_FN static inline __attribute__((always_inline)) constexpr     /* host and device under hipcc */
#else
#define WARP_FN static inline __attribute__((always_inline))
#endif

/* the four taps of one output: tap 2 dy + dx is the sample (x[dx], y[dy]) with
 * weight (dx ? fx : 256 - fx) * (dy ? fy : 256 - fy); bit 2 dy + dx of mask:
 * the tap is a sample of the window (else the plane's pad sample) */
typedef struct { int fx, fy, x[2], y[2], mask; } warp_tap;

/* the position on one axis of output (i, j): a j + b i + c */
WARP_FN int64_t warp_pos(int a, int b, int c, int i, int j)
{
    return (int64_t)a * j + (int64_t)b * i + c;
}

/* the first tap of position P on an axis of n samples, saturated to [-2, n] */
WARP_FN int warp_first(int64_t P, int n)
{
    const int64_t q = (P + 128) >> 16;
    return (int)(q < -2 ? -2 : q > n ? n : q);
}

WARP_FN int warp_frac(int64_t P)
{
    return (int)(((P + 128) >> 8) & 255);
}

WARP_FN int warp_clamp(int v, int n)
{
    return v < 0 ? 0 : v > n - 1 ? n - 1 : v;
}

/* bit d: tap p0 + d of an axis of n samples lies inside it */
WARP_FN int warp_inside(int p0, int n)
{
    return (p0 >= 0 && p0 < n ? 1 : 0) | (p0 + 1 >= 0 && p0 + 1 < n ? 2 : 0);
}

/* the taps of the positions (X, Y) in a window of cw x ch samples, both >= 1 */
WARP_FN warp_tap warp_taps_at(int64_t X, int64_t Y, int cw, int ch, int border)
{
    const int x0 = warp_first(X, cw), y0 = warp_first(Y, ch);
    const int mx = warp_inside(x0, cw), my = warp_inside(y0, ch);
    const warp_tap t = {warp_frac(X), warp_frac(Y), {warp_clamp(x0, cw), warp_clamp(x0 + 1, cw)},
                        {warp_clamp(y0, ch), warp_clamp(y0 + 1, ch)},
                        border == H264MI_WARP_BORDER_REPLICATE ? 15 : (my & 1 ? mx : 0) | (my & 2 ? mx << 2 : 0)};
    return t;
}

/* the taps of output (row i, column j) under the matrix m[0..5] */
WARP_FN warp_tap warp_taps(const int *m, int i, int j, int cw, int ch, int border)
{
    return warp_taps_at(warp_pos(m[0], m[1], m[2], i, j), warp_pos(m[3], m[4], m[5], i, j), cw, ch, border);
}

/* Outputs rows [i0, i1] x columns [j0, j1] all lie outside the window by more
 * than one sample on one side: the positions are affine in (i, j) and the first
 * tap is monotone in the position, so the four corners on one side of the
 * window put every output between them there.  (Four corners outside on
 * different sides say nothing: the tile may span the window.) */
WARP_FN int warp_tile_outside(const int *m, int i0, int i1, int j0, int j1, int cw, int ch)
{
    int lx = 1, hx = 1, ly = 1, hy = 1;
    for (int k = 0; k < 4; k++) {
        const int i = k & 2 ? i1 : i0, j = k & 1 ? j1 : j0;
        const int x0 = warp_first(warp_pos(m[0], m[1], m[2], i, j), cw);
        const int y0 = warp_first(warp_pos(m[3], m[4], m[5], i, j), ch);
        lx &= x0 < -1; hx &= x0 >= cw; ly &= y0 < -1; hy &= y0 >= ch;
    }
    return lx | hx | ly | hy;
}

#endif
