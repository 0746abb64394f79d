// engine_priv.h -- what the engine's two translation units share: engine.hip
// (the reconstruction core: creation, launch policy, decode paths, timing,
// concealment) and exports.hip (every export kernel's entry points and the
// retention state they read).  Host-only; not part of the C-ABI, and not the
// adapter's interface (engine_int.h).
//
// The core reaches the export side through the three hooks at the end and
// nowhere else; the export side uses the core's members of the struct (frame
// slots, records, stream) and the public h264mi_engine_* calls.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../../include/h264mi.h"
#include "../../../include/h264mi_records.h"

#define HIPCHECK(x)                                                                    \
    do {                                                                               \
        hipError_t err_ = (x);                                                         \
        if (err_ != hipSuccess) {                                                      \
            fprintf(stderr, "h264mi: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(err_), \
                    __FILE__, __LINE__);                                               \
            return -1;                                                                 \
        }                                                                              \
    } while (0)

// the export side's state (exports.hip owns every member; zeroed with the engine)
struct engine_exports {
    uint8_t *d_rgba;          // h264mi_engine_read_rgba / _read_crop staging (w*h*4 B, allocated on first use)
    hipEvent_t ev_exp_in, ev_exp_out;   // export_ordered, every export into the caller's memory: the caller's stream -> ours -> the caller's (created on first use)
    MbRec *d_keep;            // h264mi_engine_keep_records: per (stream, slot) the records of the last reconstruction into it (NULL: off),
                              // and one more batch that stays 0xFF ("no information")
    int keep_rec;             // the caller's own switch (d_keep is also held while d_keepc is)
    int16_t *d_keepc;         // h264mi_engine_keep_coefs: per (stream, slot) that reconstruction's coefficient blocks (NULL: off)
    uint8_t *keepc_ok;        // per (stream, slot): d_keepc holds the blocks d_keep's records index (host)
    uint32_t *d_acc;          // h264mi_engine_keep_accmv: per (stream, slot) the origin map of the last reconstruction into it (NULL: off)
    unsigned long long *acc_key;  // per stream: serial of its current key picture (host; 0: none yet)
    unsigned long long *acc_ser;  // per (stream, slot): the key serial its map was written under (host; 0: no map)
    uint8_t *d_akey;          // h264mi_engine_keep_accres: per (stream, entry < akey_n) a key picture's frame (NULL: off)
    int akey_n;               // entries per stream (0: off)
    unsigned long long *akey_tag; // per (stream, entry): the key serial whose picture the entry holds (host; 0: none)
    int *akey_slot;           // per stream: the slot its current key picture sits in (host; -1: none, or written over)
};

struct h264mi_engine {
    int dev;
    int w, h, nmbs, nstreams, nslots;
    size_t frame_bytes;           // device slot stride (H264MI_SLOT_BYTES: chroma rows padded to 128 B)
    size_t pic_bytes;             // packed I420 picture (what leaves the device)
    int cpitch;                   // chroma row pitch in a slot (H264MI_CPITCH)
    uint8_t *d_frames;
    unsigned long long *d_mbx;    // row mailboxes: 32 granules (256 B) per batch MB
    unsigned epoch;
    unsigned long long *d_prof;   // optional per-MB chain stamps (profiling k_wgpp)
    size_t prof_cap;
    int pipe_cap;                 // pictures per launch the per-picture buffers hold
    unsigned long long *d_gjunk;  // 64 KiB store sink (ReconArgs::gjunk)
    const char *last_kernel;      // name of the last batch's reconstruction kernel (diagnostics)
    int last_dep;                 // the last batch's dependency mode (DEP_NONE / DEP_ROWS / DEP_COLS)
    int last_nmc;                 // the last batch's MC waves per row workgroup
    uint8_t *d_dbrec;         // 64 B per batch MB (x2: k_prep double buffer)
    int16_t *d_res;           // 384 x int16 per batch MB (x2)
    // k_prep (deblocking records + residuals) writes buffer half prep_parity;
    // a batch prepped by the previous launch's tail workgroups is `prepped`
    int prep_parity;
    int conceal_fits;                         // k_conceal's per-MB flags fit its LDS
    const void *prepped_rec, *prepped_pics;
    int prepped_n;                            // pictures the tail prepped
    unsigned long long *d_rows_done;   // row workgroups finished, all launches (tail-prep trigger)
    // k_conceal inputs (order + decoded flags): pinned staging, device copy,
    // and an event after the upload (the staging's reuse waits for it)
    uint8_t *h_conceal, *d_conceal;
    hipEvent_t ev_conceal;
    int prep_wgs;                      // tail workgroups per launch (H264MI_PREP_WGS, default 2048)
    unsigned long long rows_launched;
    int prep_at_pct;                   // tail prep waits for this % of the launch's rows (H264MI_PREP_AT; 0: no wait)
    int mc_waves;                      // MC waves per row workgroup: 0 = per launch (below), 2, 3 or 6 forced (H264MI_MC_WAVES)
    int intra_mc6;                     // intra-heavy launches may take 6 MC waves (launch_nmc; H264MI_INTRA_MC6=0: 3)
    int launch_intra;                  // next launch: 1 = has an intra-heavy picture, 0 = none, -1 = unknown
    int dep_mode;                      // frame-pipelined launches: DEP_ROWS / DEP_COLS (H264MI_DEP_MODE; default rows)
    int launch_dep;                    // next launch's mode (h264mi_engine_hint_deps), 0 = dep_mode
    int rpw_max;                       // MB rows per k_wgpp workgroup allowed by LDS, 1..3
    int rpw_env;                       // H264MI_RPW: fixed rows per workgroup (0: by batch size)
    int ncu;
    MbRec *d_rec;
    int16_t *d_coef;
    size_t coef_cap;          // blocks
    PicDesc *d_pics;
    unsigned *d_err;
    MbRec *h_rec;             // pinned staging
    int16_t *h_coef;
    size_t h_coef_cap;
    PicDesc *h_pics;
    unsigned *h_err;
    hipStream_t st;
    hipEvent_t ev_staged, ev0, ev1, ev2;
    hipEvent_t ev_block;      // H264MI_BLOCKING_SYNC: h264mi_engine_sync sleeps on this event
    uint32_t err_accum;
    int timing;
    // per-batch kernel timing (h264mi_engine_set_timing): event triples
    hipEvent_t *tev;
    int tev_cap, tev_n;
    int tev_stride, tev_seq;  // record every tev_stride-th launch (h264mi_engine_set_timing_stride)
    engine_exports exp;       // the core touches it only through the hooks below
    int steps;                // pictures per stream per launch (h264mi_engine_set_steps)
    unsigned long long *d_prog;   // per picture row of a launch, per row wave: {MBs stored, epoch} (frame-pipelined launches)
    unsigned *d_done;             // per picture row of a launch: epoch once the row is stored
    int check;                // H264MI_CHECK=1: the dependency-checker kernels (recon_kernels.hip CHK_*)
    int check_inject;         // H264MI_CHECK_INJECT: test hook (ReconArgs::chk_inject)
    int check_short_cols, check_short_rows;   // H264MI_CHECK_INJECT_REFCOLS / _REFROWS: test hooks
    uint32_t err_bits;        // OR of every picture's device flags since the last h264mi_engine_error_bits
};

// -------- the core's hooks into the export side (exports.hip) --------
#define ENGINE_HIDDEN __attribute__((visibility("hidden")))
// what is kept of the uploaded batch (records, coefficients, origin maps, key
// pictures), queued on the engine's stream behind the batch's launch: picture
// i of the npics went into slot cur_slot[i] of stream[i]; recs[i] are its host
// records, ncoef[i] its coefficient blocks in d_coef
ENGINE_HIDDEN int engine_exports_retain(h264mi_engine *e, int npics, const int *stream, const int *cur_slot,
                                        const void *const *recs, const uint32_t *ncoef);
// the slot's samples changed after its reconstruction (k_conceal): a key
// picture's copy is taken again
ENGINE_HIDDEN int engine_exports_slot_changed(h264mi_engine *e, int stream, int slot);
// frees everything the export side holds (h264mi_engine_destroy, the stream idle)
ENGINE_HIDDEN void engine_exports_free(h264mi_engine *e);
