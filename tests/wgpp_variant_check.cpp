// k_wgpp's variant list and selection (broadway_amd/csrc/hip/wgpp_variants.h)
// on the CPU: every launch shape the engine can produce (launch_batch:
// rows_per_wg, launch_nmc, the dependency mode) against the expected rows
// written out below -- the instance, the diagnostic name, where the timing
// events go -- and the shapes it cannot produce, which must find no instance.
// Prints one line per input and "ok ..." at the end; a mismatch is reported on
// stderr and fails the run.  tests/test_wgpp_variants.py builds this with
// AddressSanitizer + UBSan.
#include <stdio.h>
#include <string.h>

#include "../broadway_amd/csrc/hip/wgpp_variants.h"

static const bool F = false, T = true;
enum { PACKET = 1, AROUND = 0 };

struct Row {
    bool dep3;
    int dmode;              // frame-pipelined rows: the launch's mode (single-step rows: every mode is walked)
    int nmc, rpw;
    bool prof, check;
    WgppVariant want;       // {NMC, PROF, RPW, CHK, DEPM}
    const char *name;
    int events;
};

static const Row rows[] = {
    // frame-pipelined: single-row, 2 MC waves; the checker wins over profiling
    {T, DEP_ROWS, 2, 1, F, F, {2, F, 1, F, DEP_ROWS}, "k_wgpp", PACKET},
    {T, DEP_ROWS, 2, 1, T, F, {2, T, 1, F, DEP_ROWS}, "k_wgpp_prof", PACKET},
    {T, DEP_ROWS, 2, 1, F, T, {2, F, 1, T, DEP_ROWS}, "k_wgpp_check", PACKET},
    {T, DEP_ROWS, 2, 1, T, T, {2, F, 1, T, DEP_ROWS}, "k_wgpp_check", PACKET},
    {T, DEP_COLS, 2, 1, F, F, {2, F, 1, F, DEP_COLS}, "k_wgpp", PACKET},
    {T, DEP_COLS, 2, 1, T, F, {2, T, 1, F, DEP_COLS}, "k_wgpp_prof", PACKET},
    {T, DEP_COLS, 2, 1, F, T, {2, F, 1, T, DEP_COLS}, "k_wgpp_check", PACKET},
    {T, DEP_COLS, 2, 1, T, T, {2, F, 1, T, DEP_COLS}, "k_wgpp_check", PACKET},
    // single step, plain
    {F, 0, 3, 1, F, F, {3, F, 1, F, DEP_NONE}, "k_wgpp", PACKET},
    {F, 0, 3, 2, F, F, {3, F, 2, F, DEP_NONE}, "k_wgpp", PACKET},
    {F, 0, 3, 3, F, F, {3, F, 3, F, DEP_NONE}, "k_wgpp", PACKET},
    {F, 0, 2, 1, F, F, {2, F, 1, F, DEP_NONE}, "k_wgpp", PACKET},
    {F, 0, 2, 2, F, F, {2, F, 2, F, DEP_NONE}, "k_wgpp", PACKET},
    {F, 0, 6, 1, F, F, {6, F, 1, F, DEP_NONE}, "k_wgpp", PACKET},
    // single step, profiling: two rows per workgroup run the 3-wave build whatever nmc
    {F, 0, 3, 1, T, F, {3, T, 1, F, DEP_NONE}, "k_wgpp", AROUND},
    {F, 0, 3, 2, T, F, {3, T, 2, F, DEP_NONE}, "k_wgpp", AROUND},
    {F, 0, 3, 3, T, F, {3, T, 3, F, DEP_NONE}, "k_wgpp", AROUND},
    {F, 0, 2, 1, T, F, {2, T, 1, F, DEP_NONE}, "k_wgpp", AROUND},
    {F, 0, 2, 2, T, F, {3, T, 2, F, DEP_NONE}, "k_wgpp", AROUND},
    {F, 0, 6, 1, T, F, {6, T, 1, F, DEP_NONE}, "k_wgpp", AROUND},
    // single step, checker
    {F, 0, 3, 1, F, T, {3, F, 1, T, DEP_NONE}, "k_wgpp_check", AROUND},
    {F, 0, 3, 2, F, T, {3, F, 2, T, DEP_NONE}, "k_wgpp_check", AROUND},
    {F, 0, 3, 3, F, T, {3, F, 3, T, DEP_NONE}, "k_wgpp_check", AROUND},
    {F, 0, 2, 1, F, T, {2, F, 1, T, DEP_NONE}, "k_wgpp_check", AROUND},
    {F, 0, 2, 2, F, T, {2, F, 2, T, DEP_NONE}, "k_wgpp_check", AROUND},
    {F, 0, 6, 1, F, T, {6, F, 1, T, DEP_NONE}, "k_wgpp_check", AROUND},
    // single step, profiling and checker: profiling wins
    {F, 0, 3, 1, T, T, {3, T, 1, F, DEP_NONE}, "k_wgpp", AROUND},
    {F, 0, 3, 2, T, T, {3, T, 2, F, DEP_NONE}, "k_wgpp", AROUND},
    {F, 0, 3, 3, T, T, {3, T, 3, F, DEP_NONE}, "k_wgpp", AROUND},
    {F, 0, 2, 1, T, T, {2, T, 1, F, DEP_NONE}, "k_wgpp", AROUND},
    {F, 0, 2, 2, T, T, {3, T, 2, F, DEP_NONE}, "k_wgpp", AROUND},
    {F, 0, 6, 1, T, T, {6, T, 1, F, DEP_NONE}, "k_wgpp", AROUND},
};

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, __VA_ARGS__); fprintf(stderr, " [%s]\n", #cond); } } while (0)

static bool same(const WgppVariant &a, const WgppVariant &b)
{
    return a.nmc == b.nmc && a.prof == b.prof && a.rpw == b.rpw && a.chk == b.chk && a.depm == b.depm;
}

static int chosen[WGPP_NVARIANTS];

static void walk(const Row &r, int dmode)
{
    char in[96];
    snprintf(in, sizeof(in), "%s dmode %d nmc %d rpw %d prof %d check %d", r.dep3 ? "pipelined" : "single", dmode, r.nmc,
             r.rpw, r.prof, r.check);
    const WgppChoice c = wgpp_select(r.nmc, r.rpw, r.prof, r.check, r.dep3, dmode);
    CHECK(c.variant >= 0 && c.variant < WGPP_NVARIANTS, "%s: variant %d", in, c.variant);
    if (c.variant < 0 || c.variant >= WGPP_NVARIANTS) return;
    const WgppVariant &v = wgpp_variants[c.variant];
    chosen[c.variant]++;
    printf("%s -> <%d,%d,%d,%d,%d> %s %s\n", in, v.nmc, v.prof, v.rpw, v.chk, v.depm, c.name,
           c.ev_on_packet ? "packet" : "around");
    CHECK(same(v, r.want), "%s: <%d,%d,%d,%d,%d>", in, v.nmc, v.prof, v.rpw, v.chk, v.depm);
    CHECK(c.name && !strcmp(c.name, r.name), "%s: name %s", in, c.name ? c.name : "(null)");
    CHECK(c.ev_on_packet == (r.events == PACKET), "%s: events on packet %d", in, c.ev_on_packet);
    const int block = wgpp_block_size(v.nmc, v.rpw);
    CHECK(block == 64 * (v.nmc + 2) * v.rpw && block <= 1024, "%s: block %d", in, block);
}

static void none(bool dep3, int dmode, int nmc, int rpw)
{
    for (int fl = 0; fl < 4; fl++) {
        const WgppChoice c = wgpp_select(nmc, rpw, fl & 1, fl >> 1, dep3, dmode);
        printf("%s dmode %d nmc %d rpw %d prof %d check %d -> none\n", dep3 ? "pipelined" : "single", dmode, nmc, rpw,
               fl & 1, fl >> 1);
        CHECK(c.variant == -1, "%s dmode %d nmc %d rpw %d flavour %d: variant %d", dep3 ? "pipelined" : "single", dmode,
              nmc, rpw, fl, c.variant);
    }
}

int main()
{
    static_assert(wgpp_block_size(3, 1) == 320 && wgpp_block_size(6, 1) == 512 && wgpp_block_size(3, 3) == 960, "");
    int inputs = 0;
    for (const Row &r : rows) {
        if (r.dep3) { walk(r, r.dmode); inputs++; continue; }
        // a single-step launch ignores the engine's dependency mode
        for (int dmode = DEP_ROWS; dmode <= DEP_COLS; dmode++) { walk(r, dmode); inputs++; }
    }
    // the list: no duplicates, every block size a legal one, every instance reachable
    for (int i = 0; i < WGPP_NVARIANTS; i++) {
        const WgppVariant &v = wgpp_variants[i];
        for (int k = 0; k < i; k++) CHECK(!same(v, wgpp_variants[k]), "variants %d and %d are the same", k, i);
        CHECK(wgpp_find(v.nmc, v.prof, v.rpw, v.chk, v.depm) == i, "variant %d is not found at its index", i);
        CHECK(wgpp_block_size(v.nmc, v.rpw) <= 1024, "variant %d: block %d", i, wgpp_block_size(v.nmc, v.rpw));
        CHECK(chosen[i] > 0, "variant %d <%d,%d,%d,%d,%d> is chosen by no input", i, v.nmc, v.prof, v.rpw, v.chk, v.depm);
    }
    // what launch_batch cannot ask for
    for (int dmode = DEP_ROWS; dmode <= DEP_COLS; dmode++) {
        none(false, dmode, 2, 3);
        none(false, dmode, 6, 2);
        none(false, dmode, 6, 3);
        const int waves[] = {2, 3, 6};
        for (int nmc : waves)
            for (int rpw = 1; rpw <= 3; rpw++)
                if (nmc != 2 || rpw != 1) none(true, dmode, nmc, rpw);
    }
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("ok %d inputs %d variants\n", inputs, WGPP_NVARIANTS);
    return 0;
}
