// k_wgpp's instances and the choice among them, stated once.  Plain C++17, no
// HIP: recon_kernels.hip takes the block size from here, engine.hip (the core
// unit; exports.hip never sees this list) derives from the list the kernels it
// emits, their addresses, LDS sizes and launch attributes, and
// tests/wgpp_variant_check.cpp walks the selection on the CPU.
#ifndef H264MI_WGPP_VARIANTS_H
#define H264MI_WGPP_VARIANTS_H

// dependency mode of a frame-pipelined launch (k_wgpp's DEPM)
enum { DEP_NONE = 0, DEP_ROWS = 1, DEP_COLS = 2 };

// threads of a k_wgpp workgroup: per MB row NMC MC waves and two row waves.
// The kernel's __launch_bounds__ and every launch use this one expression.
constexpr int wgpp_block_size(int nmc, int rpw) { return 64 * (nmc + 2) * rpw; }

// X(NMC, PROF, RPW, CHK, DEPM): MC waves per row, profiling stamps, MB rows
// per workgroup, dependency checker (H264MI_CHECK=1), dependency mode
#define WGPP_VARIANTS(X)                                                        \
    X(3, false, 1, false, DEP_NONE)                                             \
    X(3, false, 2, false, DEP_NONE)                                             \
    X(3, false, 3, false, DEP_NONE)                                             \
    X(2, false, 1, false, DEP_NONE)                                             \
    X(2, false, 2, false, DEP_NONE)                                             \
    /* intra-heavy single-step launches whose rows all fit two workgroups per  \
       CU: six MC waves per row (engine launch_nmc) */                          \
    X(6, false, 1, false, DEP_NONE)                                             \
    /* profiling (tools/prof_steps.py, prof_chain.py, sq_roles.py); two rows   \
       per workgroup always run the 3-wave build */                             \
    X(3, true, 1, false, DEP_NONE)                                              \
    X(3, true, 2, false, DEP_NONE)                                              \
    X(3, true, 3, false, DEP_NONE)                                              \
    X(2, true, 1, false, DEP_NONE)                                              \
    X(6, true, 1, false, DEP_NONE)                                              \
    /* dependency checker */                                                    \
    X(3, false, 1, true, DEP_NONE)                                              \
    X(3, false, 2, true, DEP_NONE)                                              \
    X(3, false, 3, true, DEP_NONE)                                              \
    X(2, false, 1, true, DEP_NONE)                                              \
    X(2, false, 2, true, DEP_NONE)                                              \
    X(6, false, 1, true, DEP_NONE)                                              \
    /* frame-pipelined launches (single-row, 2 MC waves), by dependency mode */ \
    X(2, false, 1, false, DEP_ROWS)                                             \
    X(2, false, 1, true, DEP_ROWS)                                              \
    X(2, true, 1, false, DEP_ROWS)                                              \
    X(2, false, 1, false, DEP_COLS)                                             \
    X(2, false, 1, true, DEP_COLS)                                              \
    X(2, true, 1, false, DEP_COLS)

struct WgppVariant { int nmc; bool prof; int rpw; bool chk; int depm; };
#define WGPP_VARIANT_ROW(NMC, PROF, RPW, CHK, DEPM) {NMC, PROF, RPW, CHK, DEPM},
constexpr WgppVariant wgpp_variants[] = {WGPP_VARIANTS(WGPP_VARIANT_ROW)};
#undef WGPP_VARIANT_ROW
constexpr int WGPP_NVARIANTS = sizeof(wgpp_variants) / sizeof(wgpp_variants[0]);

// index of an instance in the list, -1: not built
constexpr int wgpp_find(int nmc, bool prof, int rpw, bool chk, int depm)
{
    for (int i = 0; i < WGPP_NVARIANTS; i++) {
        const WgppVariant &v = wgpp_variants[i];
        if (v.nmc == nmc && v.prof == prof && v.rpw == rpw && v.chk == chk && v.depm == depm) return i;
    }
    return -1;
}

struct WgppChoice {
    int variant;          // index into wgpp_variants, -1: no instance serves the request
    const char *name;     // h264mi_engine_kernel's diagnostic name
    bool ev_on_packet;    // timing events ride on the kernel's dispatch packet (else recorded around the launch)
};

// The instance for a launch of nmc MC waves and rpw rows per workgroup:
// frame-pipelined (dep3, mode dmode) or single-step, with the profiling
// buffer and / or the dependency checker on.  Frame-pipelined launches are
// single-row with two MC waves and the checker wins over profiling; in a
// single-step launch profiling wins, and its two-row shape is built with
// three MC waves only.  What launch_batch never asks for (2 waves x 3 rows,
// 6 waves x several rows, a pipelined launch of another shape) has no
// instance.
inline WgppChoice wgpp_select(int nmc, int rpw, bool prof, bool check, bool dep3, int dmode)
{
    WgppChoice c = {-1, "k_wgpp", true};
    if ((nmc == 2 && rpw == 3) || (nmc == 6 && rpw > 1)) return c;
    if (dep3) {
        if (nmc != 2 || rpw != 1 || (dmode != DEP_ROWS && dmode != DEP_COLS)) return c;
        prof = prof && !check;
        c.name = check ? "k_wgpp_check" : prof ? "k_wgpp_prof" : "k_wgpp";
        c.variant = wgpp_find(2, prof, 1, check, dmode);
        return c;
    }
    if (prof) {
        check = false;
        if (rpw == 2) nmc = 3;
    }
    if (check) c.name = "k_wgpp_check";
    c.ev_on_packet = !prof && !check;
    c.variant = wgpp_find(nmc, prof, rpw, check, DEP_NONE);
    return c;
}

#endif
