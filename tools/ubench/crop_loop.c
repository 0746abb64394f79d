/* What a caller pays to crop on the host: one byte at a time, the crop window
 * of a planar I420 picture into a packed one (luma, then the two chroma
 * planes at half size) -- timed on the calling thread's CPU clock.
 * tools/crop_cost.py runs it for leg (c).
 *   crop_loop WIDTH HEIGHT X Y CW CH REPS  -> "crop_loop_cpu_us_per_picture N" */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

/* plane: pw bytes per row; its window at (px, py), ww x wh; returns the end of the output */
static uint8_t *plane_bytes(uint8_t *out, const uint8_t *plane, size_t pw, size_t px, size_t py, size_t ww, size_t wh)
{
    for (size_t r = 0; r < wh; r++)
        for (size_t c = 0; c < ww; c++)
            out[r * ww + c] = plane[(py + r) * pw + px + c];
    return out + ww * wh;
}

static void crop_bytes(uint8_t *out, const uint8_t *in, unsigned w, unsigned h, unsigned x, unsigned y, unsigned cw,
                       unsigned ch)
{
    const size_t ysz = (size_t)w * h, csz = ysz / 4;
    out = plane_bytes(out, in, w, x, y, cw, ch);
    out = plane_bytes(out, in + ysz, w / 2, x / 2, y / 2, cw / 2, ch / 2);
    (void)plane_bytes(out, in + ysz + csz, w / 2, x / 2, y / 2, cw / 2, ch / 2);
}

int main(int argc, char **argv)
{
    if (argc < 8) return 2;
    const unsigned w = atoi(argv[1]), h = atoi(argv[2]), x = atoi(argv[3]), y = atoi(argv[4]), cw = atoi(argv[5]),
                   ch = atoi(argv[6]), reps = atoi(argv[7]);
    if (!reps || x + cw > w || y + ch > h) return 2;
    /* several pictures in rotation, as a decoder's output frames are: no picture stays in L2 */
    enum { NPIC = 8 };
    uint8_t *in = malloc((size_t)w * h * 3 / 2 * NPIC), *out = malloc((size_t)cw * ch * 3 / 2);
    if (!in || !out) return 1;
    for (size_t i = 0; i < (size_t)w * h * 3 / 2 * NPIC; i++) in[i] = (uint8_t)(i * 131);
    struct timespec a, b;
    volatile unsigned sink = 0;
    crop_bytes(out, in, w, h, x, y, cw, ch);
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &a);
    for (unsigned r = 0; r < reps; r++) {
        crop_bytes(out, in + (size_t)(r % NPIC) * w * h * 3 / 2, w, h, x, y, cw, ch);
        sink += out[r % 97];
    }
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &b);
    printf("crop_loop_cpu_us_per_picture %.2f\n",
           ((double)(b.tv_sec - a.tv_sec) * 1e6 + (double)(b.tv_nsec - a.tv_nsec) * 1e-3) / reps);
    free(in); free(out);
    return 0;
}
