// h264mi engine: HBM-resident frame slots, record upload, kernel launches.
// One engine serves `nstreams` independent bitstreams of one picture size
// (streams shard across GPUs with no collective; within a GPU
// one launch reconstructs one picture from each stream of the batch).
#include "recon_kernels.hip"
#include "color.hip"
#include "crop.hip"
#include "tensor.hip"
#include "resize.hip"
#include "field_store.h"
#include "mbinfo.hip"
#include "residual.hip"
#include "accmv.hip"
#include "accres.hip"
#include "field_resize.hip"
#include "conceal.hip"
#include <hip/hip_ext.h>

#include <stdio.h>
#include <atomic>
#include <vector>
#include <stdlib.h>
#include <string.h>
#include "../../../include/h264mi.h"
#include "../common/export_desc.h"
#include "engine_int.h"

#define HIPCHECK(x)                                                                    \
    do {                                                                               \
        hipError_t err_ = (x);                                                         \
        if (err_ != hipSuccess) {                                                      \
            fprintf(stderr, "h264mi: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(err_), \
                    __FILE__, __LINE__);                                               \
            return -1;                                                                 \
        }                                                                              \
    } while (0)

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
    int steps;                // pictures per stream per launch (h264mi_engine_set_steps)
    unsigned long long *d_prog;   // per picture row of a launch, per row wave: {MBs stored, epoch} (frame-pipelined launches)
    unsigned *d_done;             // per picture row of a launch: epoch once the row is stored
    int check;                // H264MI_CHECK=1: the dependency-checker kernels (recon_kernels.hip CHK_*)
    int check_inject;         // H264MI_CHECK_INJECT: test hook (ReconArgs::chk_inject)
    int check_short_cols, check_short_rows;   // H264MI_CHECK_INJECT_REFCOLS / _REFROWS: test hooks
    uint32_t err_bits;        // OR of every picture's device flags since the last h264mi_engine_error_bits
};

// k_wgpp's instances, in the order of wgpp_variants (wgpp_variants.h): this
// table is what instantiates them.  lds: the dynamic LDS of a launch on a
// picture w MBs wide (cols: a DEP_COLS launch's progress cache beside it)
struct WgppLaunch {
    const void *fn;
    size_t (*lds)(int w, bool cols);
};
#define WGPP_LAUNCH_ROW(NMC, PROF, RPW, CHK, DEPM) \
    {reinterpret_cast<const void *>(&k_wgpp<NMC, PROF, true, RPW, CHK, DEPM>), &WgppLds<NMC, RPW>::bytes},
static const WgppLaunch wgpp_launch[WGPP_NVARIANTS] = {WGPP_VARIANTS(WGPP_LAUNCH_ROW)};
#undef WGPP_LAUNCH_ROW

// per-picture buffers of one launch (deblocking records, residuals, row
// mailboxes, error flags), for `cap` pictures
static void free_pic_buffers(h264mi_engine *e)
{
    (void)hipFree(e->d_mbx); (void)hipFree(e->d_dbrec); (void)hipFree(e->d_res); (void)hipFree(e->d_err);
    (void)hipFree(e->d_prog);
    (void)hipFree(e->d_done);
    (void)hipHostFree(e->h_err);
    e->d_mbx = NULL; e->d_dbrec = NULL; e->d_res = NULL; e->d_err = NULL; e->d_prog = NULL; e->d_done = NULL;
    e->h_err = NULL;
    e->pipe_cap = 0;
}

static int alloc_pic_buffers(h264mi_engine *e, int cap)
{
    const size_t np = (size_t)cap, mbs = np * e->nmbs;
    bool ok = hipMalloc(&e->d_mbx, mbs * 256) == hipSuccess &&
              hipMalloc(&e->d_dbrec, 2 * mbs * 64) == hipSuccess &&
              hipMalloc(&e->d_res, 2 * mbs * 768) == hipSuccess &&
              hipMalloc(&e->d_err, sizeof(unsigned) * np) == hipSuccess &&
              hipMalloc(&e->d_prog, sizeof(unsigned long long) * 2 * PROG_STRIDE * np * e->h) == hipSuccess &&
              hipMalloc(&e->d_done, sizeof(unsigned) * np * e->h) == hipSuccess &&
              hipHostMalloc(&e->h_err, sizeof(unsigned) * np, hipHostMallocDefault) == hipSuccess;
    if (!ok) { free_pic_buffers(e); return -1; }
    // cleared granules carry epoch 0, which no launch uses
    (void)hipMemsetAsync(e->d_mbx, 0, mbs * 256, e->st);
    (void)hipMemsetAsync(e->d_err, 0, sizeof(unsigned) * np, e->st);
    (void)hipMemsetAsync(e->d_prog, 0, sizeof(unsigned long long) * 2 * PROG_STRIDE * np * e->h, e->st);
    (void)hipMemsetAsync(e->d_done, 0, sizeof(unsigned) * np * e->h, e->st);
    memset(e->h_err, 0, sizeof(unsigned) * np);
    e->pipe_cap = cap;
    return 0;
}

// settings read from the environment at engine creation (and again when a
// pooled engine is taken for a new decoder instance)
static void engine_config(h264mi_engine *e)
{
    e->timing = getenv("H264MI_TIMING") != NULL;
    const char *pw = getenv("H264MI_PREP_WGS");
    e->prep_wgs = pw && atoi(pw) > 0 ? atoi(pw) : 2048;
    const char *pa = getenv("H264MI_PREP_AT");
    e->prep_at_pct = pa ? atoi(pa) : 0;
    const char *mw = getenv("H264MI_MC_WAVES");
    e->mc_waves = mw && (atoi(mw) == 2 || atoi(mw) == 3 || atoi(mw) == 6) ? atoi(mw) : 0;
    const char *m6 = getenv("H264MI_INTRA_MC6");
    e->intra_mc6 = m6 ? atoi(m6) != 0 : 1;
    e->launch_intra = -1;
    {
        const char *dm = getenv("H264MI_DEP_MODE");
        e->dep_mode = dm && (!strcmp(dm, "cols") || atoi(dm) == DEP_COLS) ? DEP_COLS : DEP_ROWS;
        e->launch_dep = 0;
    }
    e->check = getenv("H264MI_CHECK") && atoi(getenv("H264MI_CHECK"));
    e->check_inject = h264mi_test_hooks() && getenv("H264MI_CHECK_INJECT") ? atoi(getenv("H264MI_CHECK_INJECT")) : 0;
    e->check_short_cols = h264mi_test_hooks() && getenv("H264MI_CHECK_INJECT_REFCOLS") ? atoi(getenv("H264MI_CHECK_INJECT_REFCOLS")) : 0;
    e->check_short_rows = h264mi_test_hooks() && getenv("H264MI_CHECK_INJECT_REFROWS") ? atoi(getenv("H264MI_CHECK_INJECT_REFROWS")) : 0;
    const char *rp = getenv("H264MI_RPW");
    e->rpw_env = rp ? atoi(rp) : 0;
    if (e->rpw_env < 0 || e->rpw_env > 3) e->rpw_env = 0;
    // the group's LDS mailboxes (w * 256 B per inner row boundary) beside
    // the static LDS of its rows (regions, MC scratch, a RINGG-slot ring)
    // within the CU's 160 KB
    // k_wgpp's LDS is dynamic (WgppLds): allow every variant the CU's 160 KB
    for (const WgppLaunch &k : wgpp_launch)
        (void)hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const size_t row_lds = sizeof(PPLds) + (size_t)(e->mc_waves == 2 ? 2 : e->mc_waves == 6 ? 6 : 3) * sizeof(McScratch) + sizeof(MbRing<RINGG>);
    e->rpw_max = e->mc_waves == 2 ? 2 : 3;
    while (e->rpw_max > 1 && (size_t)(e->rpw_max - 1) * e->w * 256 + (size_t)e->rpw_max * row_lds > 156 * 1024)
        e->rpw_max--;
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, e->dev) != hipSuccess || ncu < 1) ncu = 256;
    e->ncu = ncu;
    // k_conceal keeps one decoded flag per MB in dynamic LDS: up to the CU's
    // 160 KB less its static part; larger pictures conceal on the host
    // (engine_conceal_fits -> the backend's conceal_ok)
    // (one byte per MB; the attribute is raised only for pictures above the
    // default 64 KB limit (less k_conceal's static sums and headroom), so a
    // device that refuses it still conceals
    // the sizes that fit)
    e->conceal_fits = (size_t)e->nmbs <= 60 * 1024 ||
                      ((size_t)e->nmbs <= CONCEAL_LDS_MAX &&
                       hipFuncSetAttribute(reinterpret_cast<const void *>(&k_conceal),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, CONCEAL_LDS_MAX) == hipSuccess);
}

extern "C" h264mi_engine *h264mi_engine_create(int device, int w_mbs, int h_mbs, int nstreams, int nslots)
{
    if (w_mbs < 1 || h_mbs < 1 || h_mbs > 1024 || nstreams < 1 || nslots < 1) return NULL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
        fprintf(stderr, "h264mi: no HIP device %d (count %d)\n", device, ndev);
        return NULL;
    }
    if (hipSetDevice(device) != hipSuccess) return NULL;
    // H264MI_BLOCKING_SYNC=1: a thread waiting for the GPU sleeps instead of
    // spinning (many decoder processes with parse threads on few host cores)
    const bool blocking = getenv("H264MI_BLOCKING_SYNC") && atoi(getenv("H264MI_BLOCKING_SYNC"));
    if (blocking) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
    h264mi_engine *e = (h264mi_engine *)calloc(1, sizeof(h264mi_engine));
    if (!e) return NULL;
    e->dev = device;
    e->w = w_mbs; e->h = h_mbs; e->nmbs = w_mbs * h_mbs;
    e->nstreams = nstreams; e->nslots = nslots;
    e->steps = 1;
    e->frame_bytes = H264MI_SLOT_BYTES(w_mbs, h_mbs);
    e->pic_bytes = (size_t)e->nmbs * 384;
    e->cpitch = H264MI_CPITCH(w_mbs);
    e->coef_cap = (size_t)nstreams * e->nmbs * 8 + 1024;
    e->h_coef_cap = e->coef_cap;
    bool ok = hipMalloc(&e->d_frames, e->frame_bytes * nslots * nstreams) == hipSuccess &&

              hipMalloc(&e->d_rec, sizeof(MbRec) * nstreams * e->nmbs) == hipSuccess &&
              hipMalloc(&e->d_coef, e->coef_cap * 32) == hipSuccess &&
              hipMalloc(&e->d_pics, sizeof(PicDesc) * nstreams) == hipSuccess &&
              hipMalloc(&e->d_gjunk, 65536) == hipSuccess &&

              hipHostMalloc(&e->h_rec, sizeof(MbRec) * nstreams * e->nmbs, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc(&e->h_coef, e->h_coef_cap * 32, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc(&e->h_pics, sizeof(PicDesc) * nstreams, hipHostMallocDefault) == hipSuccess &&

              hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&e->ev_staged, hipEventDisableTiming | (blocking ? hipEventBlockingSync : 0)) == hipSuccess &&
              hipEventCreate(&e->ev0) == hipSuccess && hipEventCreate(&e->ev1) == hipSuccess &&
              hipEventCreate(&e->ev2) == hipSuccess &&
              (!blocking || hipEventCreateWithFlags(&e->ev_block, hipEventDisableTiming | hipEventBlockingSync) == hipSuccess) &&
              hipMalloc(&e->d_rows_done, sizeof(unsigned long long)) == hipSuccess;
    ok = ok && alloc_pic_buffers(e, nstreams) == 0;
    if (!ok) {
        fprintf(stderr, "h264mi: engine allocation failed\n");
        h264mi_engine_destroy(e);
        return NULL;
    }
    (void)hipMemsetAsync(e->d_frames, 0, e->frame_bytes * nslots * nstreams, e->st);
    (void)hipMemsetAsync(e->d_rows_done, 0, sizeof(unsigned long long), e->st);
    engine_config(e);
    e->epoch = 0;
    (void)hipEventRecord(e->ev_staged, e->st);
    (void)hipStreamSynchronize(e->st);
    return e;
}

extern "C" void h264mi_engine_destroy(h264mi_engine *e)
{
    if (!e) return;
    if (e->st) (void)hipStreamSynchronize(e->st);
    free_pic_buffers(e);
    (void)hipFree(e->d_rgba);
    (void)hipFree(e->d_keep);
    (void)hipFree(e->d_keepc);
    free(e->keepc_ok);
    (void)hipFree(e->d_acc);
    free(e->acc_key);
    free(e->acc_ser);
    (void)hipFree(e->d_akey);
    free(e->akey_tag);
    free(e->akey_slot);
    (void)hipFree(e->d_frames); (void)hipFree(e->d_prof); (void)hipFree(e->d_rec); (void)hipFree(e->d_coef);
    (void)hipFree(e->d_pics); (void)hipFree(e->d_gjunk);
    (void)hipHostFree(e->h_rec); (void)hipHostFree(e->h_coef); (void)hipHostFree(e->h_pics);
    if (e->ev_staged) (void)hipEventDestroy(e->ev_staged);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->ev2) (void)hipEventDestroy(e->ev2);
    if (e->ev_block) (void)hipEventDestroy(e->ev_block);
    (void)hipFree(e->d_rows_done);
    if (e->h_conceal) (void)hipHostFree(e->h_conceal);
    if (e->d_conceal) (void)hipFree(e->d_conceal);
    if (e->ev_conceal) (void)hipEventDestroy(e->ev_conceal);
    if (e->ev_exp_in) (void)hipEventDestroy(e->ev_exp_in);
    if (e->ev_exp_out) (void)hipEventDestroy(e->ev_exp_out);
    h264mi_engine_set_timing(e, 0);
    if (e->st) (void)hipStreamDestroy(e->st);
    free(e);
}

// k_prep of a batch as its own launch (the batch was not prepped by the
// previous launch's tail): deblocking records + residuals into buffer half hb
static int launch_prep(h264mi_engine *e, int npics, const MbRec *d_rec, const int16_t *d_coef,
                       const PicDesc *d_pics, int hb)
{
    const size_t mbs = (size_t)e->pipe_cap * e->nmbs;
    PrepArgs pa;
    pa.rec = d_rec; pa.coef = d_coef; pa.pics = d_pics;
    pa.dbrec = e->d_dbrec + hb * mbs * 64;
    pa.res = e->d_res + hb * mbs * 384;
    pa.nmbs_total = npics * e->nmbs;
    pa.w = e->w; pa.h = e->h;
    hipLaunchKernelGGL(k_prep, dim3((pa.nmbs_total + 3) / 4), dim3(256), 0, e->st, pa);
    HIPCHECK(hipGetLastError());
    return 0;
}

// One reconstruction step for a batch of npics pictures (one per stream), all
// on the engine's stream: k_prep unless the previous launch's tail already
// prepped this batch, then k_wgpp -- one workgroup per (picture, MB row): MC
// waves + ping-pong deblocking row waves -- plus, when the next batch is
// known (next_rec != NULL), tail workgroups that run the next batch's k_prep
// as this launch's rows drain.  k_prep outputs alternate between two buffer
// halves; stream order separates writer and reader.
// rows per workgroup: while the batch's rows fit the chip as single-row
// workgroups (three per CU), one row each -- a picture's latency is the
// bound and three chains on one CU contend; beyond that, three rows per
// workgroup with LDS hand-offs inside (measured, 1080p: S = 8 410 vs 440 us
// per launch; S = 32 1368 vs 1113 us).  H264MI_RPW fixes it; the LDS budget
// (rpw_max) and the 2-MC-wave builds cap it.
static int rows_per_wg(const h264mi_engine *e, int S)
{
    int rpw = e->rpw_env ? e->rpw_env : (S * e->h > 3 * e->ncu ? 3 : 1);
    if (rpw > e->rpw_max) rpw = e->rpw_max;
    if (e->mc_waves == 2 && rpw > 2) rpw = 2;
    if (e->mc_waves == 6) rpw = 1;
    return rpw;
}

// MC waves per single-row workgroup, per launch.  Three MC waves make a
// 5-wave workgroup, admitted 2 per CU (tools/ubench/census.hip): a 1080p
// picture's rows 64..67 then wait ~180 us for a slot, but intra pictures,
// whose MC is the critical path, need the third wave.  Two make a 4-wave
// workgroup, 3 per CU, every row resident from the start; with the MC
// urgency priority (recon_kernels.hip mc_row) P pictures gain (measured,
// configs[3] P-only: 350 vs 355 us per launch; a launch with an I picture:
// ~40 us slower).  So: 2 unless the launch holds an intra-heavy picture
// (more than half its MBs intra) or its content is unknown.  A launch of
// two steps per stream always takes 2: twice the rows compete for workgroup
// slots, and 768 of them beat the third wave even with an IDR among the
// pictures (configs[3] GOP mix: launches holding an IDR 671 vs 754 us,
// profiles/r75_ab_idr_second.txt).  An intra-heavy launch whose rows all fit
// two 8-wave workgroups per CU takes six MC waves: an intra row's pace is its
// MC waves' throughput (each wave holds an MB through the left-neighbour
// waits of its 4x4 blocks), 720p I pictures 341.6 / 324.0 / 320.2 / 316.7 us
// with 3 / 4 / 5 / 6 (profiles/r162_*, r163_*); above that the rows would
// wait for slots.
static int launch_nmc(const h264mi_engine *e, int rpw, int P, int npics)
{
    if (e->mc_waves) return e->mc_waves;
    if (rpw > 1) return 3;
    if (P > 1) return 2;
    if (e->launch_intra == 0) return 2;
    return e->launch_intra > 0 && e->intra_mc6 && npics * e->h <= 2 * e->ncu ? 6 : 3;
}

static int launch_batch(h264mi_engine *e, int S, int P, const MbRec *d_rec, const int16_t *d_coef,
                        const PicDesc *d_pics, const MbRec *next_rec, const int16_t *next_coef,
                        const PicDesc *next_pics, int next_npics = -1)
{
    const int npics = S * P;
    const size_t mbs = (size_t)e->pipe_cap * e->nmbs;
    const int hb = e->prep_parity;
    // study knob (H264MI_NO_TAIL_PREP=1): every batch's k_prep as its own
    // launch in front of k_wgpp, none in the tail -- k_wgpp's time without
    // the next batch's prep work beside the chain
    static const bool no_tail = getenv("H264MI_NO_TAIL_PREP") && atoi(getenv("H264MI_NO_TAIL_PREP"));
    if (no_tail) next_rec = nullptr, next_coef = nullptr, next_pics = nullptr;
    if (next_npics < 0) next_npics = npics;
    if (!(e->prepped_rec && e->prepped_rec == (const void *)d_rec && e->prepped_pics == (const void *)d_pics &&
          e->prepped_n == npics))
        if (launch_prep(e, npics, d_rec, d_coef, d_pics, hb)) return -1;
    ReconArgs a;
    memset(&a, 0, sizeof(a));
    a.frames = e->d_frames;
    a.frame_bytes = e->frame_bytes;
    a.cpitch = e->cpitch;
    a.rec = d_rec;
    a.coef = d_coef;
    a.mbx = e->d_mbx;
    a.gjunk = e->d_gjunk;
    if (++e->epoch >= (1u << 20)) {           // granule tags: epoch in the high dword
        if (h264mi_engine_sync(e)) return -1;
        HIPCHECK(hipMemsetAsync(e->d_mbx, 0, mbs * 256, e->st));
        HIPCHECK(hipMemsetAsync(e->d_prog, 0, sizeof(unsigned long long) * 2 * PROG_STRIDE * e->pipe_cap * e->h, e->st));
        HIPCHECK(hipMemsetAsync(e->d_done, 0, sizeof(unsigned) * e->pipe_cap * e->h, e->st));
        e->epoch = 1;
    }
    a.epoch = e->epoch;
    // (a launch of more pictures than the stamp buffer holds runs unstamped)
    a.prof = e->d_prof && (size_t)npics * ((size_t)e->h * PROF_ROW + (size_t)e->nmbs * PROF_MB) <= e->prof_cap ? e->d_prof : nullptr;
    a.prof_mode = e->d_prof && getenv("H264MI_PROF_MODE") ? atoi(getenv("H264MI_PROF_MODE")) : 0;
    // study knobs: MC lead over the row's deblocking (MBs; 0 / unset = the
    // ring depth), before the chain has begun (LEAD0, at least 4) and after
    static const int mc_lead0 = getenv("H264MI_MC_LEAD0") ? std::max(4, atoi(getenv("H264MI_MC_LEAD0"))) : 0;
    static const int mc_lead = getenv("H264MI_MC_LEAD") ? std::max(4, atoi(getenv("H264MI_MC_LEAD"))) : 0;
    a.mc_lead0 = mc_lead0;
    a.mc_lead = mc_lead;
    // row waves at s_setprio 1 off the chain (slot waits, copy-in, frame
    // stores) and 3 on it: on by default since the 4-workgroups-per-CU shape
    // (profiles/r85_ab_row_prio.txt: 305.3 vs 307.3 us per step, 6 of 6
    // rounds); H264MI_ROW_PRIO=0 turns it off
    static const int row_prio = getenv("H264MI_ROW_PRIO") ? atoi(getenv("H264MI_ROW_PRIO")) : 1;
    a.row_prio_split = row_prio;
    // the 2-MC-wave urgency distance (MBs; H264MI_MC_URGENCY): 8, and 12 in
    // launches of three or more steps (profiles/r93_ab_knobs_pipe3.txt: 303.0
    // vs 303.9 us per step, 4 of 4 rounds)
    static const int mc_urg = getenv("H264MI_MC_URGENCY") ? atoi(getenv("H264MI_MC_URGENCY")) : 0;
    a.mc_urgency = mc_urg > 0 ? mc_urg : P > 2 ? 12 : 8;
    // study knob: the top MB rows' urgent MC waves at the row waves' priority
    // (H264MI_MC_TOP rows; 0 = off)
    static const int mc_top = getenv("H264MI_MC_TOP") ? atoi(getenv("H264MI_MC_TOP")) : 0;
    a.mc_top = mc_top;
    a.chk_inject = e->check ? e->check_inject : 0;
    a.chk_short_cols = e->check ? e->check_short_cols : 0;
    a.chk_short_rows = e->check ? e->check_short_rows : 0;

    a.pics = d_pics;
    a.npics = npics;
    a.w = e->w; a.h = e->h;
    a.err = e->d_err;
    a.S = S;
    // study build only (-DSTUDY_NODEP; output NOT valid): the steps of a
    // launch wait on nothing -- the overlap an exact finer-grained dependency
    // could reach at most.  A compile-time switch, like
    // STUDY_NEAR: no environment variable changes what the library computes
#ifdef STUDY_NODEP
    a.P = 1;
#else
    a.P = P;
#endif
    a.prog = e->d_prog;
    a.done = e->d_done;
    a.dbrec = e->d_dbrec + hb * mbs * 64;
    a.res = e->d_res + hb * mbs * 384;
    const int rows = npics * e->h;
    if (next_rec) {
        a.prep_wgs = e->prep_wgs;
        a.rows_done = e->d_rows_done;
        a.prep_target = e->rows_launched + (unsigned long long)((long long)rows * e->prep_at_pct / 100);
        a.n_rec = next_rec; a.n_coef = next_coef; a.n_pics = next_pics;
        a.n_dbrec = e->d_dbrec + (hb ^ 1) * mbs * 64;
        a.n_res = e->d_res + (hb ^ 1) * mbs * 384;
        a.n_nmbs_total = next_npics * e->nmbs;
    } else {
        a.rows_done = e->d_rows_done;
    }
    hipEvent_t t0 = e->ev0, t2 = e->ev2;
    bool rec_tev = false;
    if (e->tev && e->tev_n < e->tev_cap && e->tev_seq++ % (e->tev_stride > 0 ? e->tev_stride : 1) == 0) {
        t0 = e->tev[3 * e->tev_n]; t2 = e->tev[3 * e->tev_n + 2];
        e->tev_n++;
        rec_tev = true;
    }
    const bool rec = e->timing || rec_tev;
    // frame-pipelined launches: the DEP_ROWS / DEP_COLS instances (single-row,
    // 2 MC waves).  The mode is the caller's hint for this launch or the
    // engine's default; whole rows need every slot below 32 (a bit mask)
    const bool dep3 = P > 1;
    int dmode = e->launch_dep ? e->launch_dep : e->dep_mode;
    if (e->nslots > 32) dmode = DEP_COLS;
    e->launch_dep = 0;                        // a hint covers one launch
    e->last_dep = dep3 ? dmode : DEP_NONE;
    const int rpw = dep3 ? 1 : rows_per_wg(e, S);
    const dim3 grid(npics * ((e->h + rpw - 1) / rpw) + a.prep_wgs);
    const int nmc = dep3 ? 2 : launch_nmc(e, rpw, P, npics);
    e->last_nmc = nmc;
    e->launch_intra = -1;                     // a hint covers one launch
    // the instance for this shape (wgpp_variants.h), its LDS and block size
    const WgppChoice ch = wgpp_select(nmc, rpw, a.prof != nullptr, e->check != 0, dep3, dmode);
    if (ch.variant < 0) {
        fprintf(stderr, "h264mi: no k_wgpp instance for %d MC waves, %d rows per workgroup, %d steps\n", nmc, rpw, P);
        return -1;
    }
    const WgppVariant &v = wgpp_variants[ch.variant];
    const WgppLaunch &k = wgpp_launch[ch.variant];
    const size_t lmbx = k.lds(e->w, v.depm == DEP_COLS);
    const dim3 block(wgpp_block_size(v.nmc, v.rpw));
    void *args[] = {&a};
    e->last_kernel = ch.name;
    if (ch.ev_on_packet) {
        // the timing events ride on the kernel's own dispatch packet
        // (hipExtLaunchKernel): no marker packets between launches
        (void)hipExtLaunchKernel(k.fn, grid, block, args, lmbx, e->st, rec ? t0 : nullptr, rec ? t2 : nullptr, 0);
    } else {
        // the profiling instances, and the dependency checker's
        // (H264MI_CHECK=1: every hand-off verified at its consumer,
        // violations in the pictures' error words), outside frame-pipelined
        // launches: the events recorded around the launch
        if (rec) (void)hipEventRecord(t0, e->st);
        (void)hipLaunchKernel(k.fn, grid, block, args, lmbx, e->st);
        if (rec) (void)hipEventRecord(t2, e->st);
    }
    HIPCHECK(hipGetLastError());
    e->rows_launched += rows;
    e->prepped_rec = next_rec;
    e->prepped_pics = next_pics;
    e->prepped_n = next_npics;
    e->prep_parity = hb ^ 1;                  // the half the next batch was (or will be) prepped into
    return 0;
}

// record retention (h264mi_engine_keep_records): the uploaded batch's records,
// picture i at d_rec + i * nmbs, into the kept batches of the slots they were
// reconstructed into -- one device-to-device copy each on the engine's stream,
// behind the upload and the launch reading them and ahead of the next upload
static int keep_batch(h264mi_engine *e, int npics, const int *stream, const int *cur_slot)
{
    for (int i = 0; i < npics; i++)
        HIPCHECK(hipMemcpyAsync(e->d_keep + ((size_t)stream[i] * e->nslots + cur_slot[i]) * e->nmbs,
                                e->d_rec + (size_t)i * e->nmbs, sizeof(MbRec) * e->nmbs, hipMemcpyDeviceToDevice, e->st));
    return 0;
}

// origin-map retention (h264mi_engine_keep_accmv): one k_accmv_step launch per
// ACCMV_STEP_PICS pictures of the uploaded batch, behind the launch that
// reconstructs them and ahead of the next upload, reading d_rec in place.
// Picture i's host records recs[i] say whether it is a key picture (no MBT_INTER
// / MBT_SKIP record): that bumps its stream's key serial.  A slot's map counts
// iff it was written under the stream's current serial; the slot being written
// counts as none (a picture does not reference its own slot).
static size_t acc_words(const h264mi_engine *e) { return (size_t)e->nmbs * 256; }
static int accmv_clear(h264mi_engine *e, size_t first, size_t n);

// Key-picture retention (h264mi_engine_keep_accres): the samples of `slot`,
// which holds the stream's current key picture (serial s = acc_key[stream]),
// into the stream's entry s % akey_n, behind everything queued on the engine's
// stream so far -- the launch that reconstructs the slot is.  An export that
// reads the entry's previous picture (serial s - akey_n) runs on the same
// stream (export_ordered), so this copy waits for it as a decode into a slot
// waits for the slot's export.
static int accres_copy_key(h264mi_engine *e, int stream, int slot)
{
    const unsigned long long s = e->acc_key[stream];
    const size_t entry = (size_t)stream * e->akey_n + (size_t)(s % (unsigned)e->akey_n);
    HIPCHECK(hipMemcpyAsync(e->d_akey + entry * e->frame_bytes,
                            e->d_frames + e->frame_bytes * ((size_t)stream * e->nslots + slot), e->frame_bytes,
                            hipMemcpyDeviceToDevice, e->st));
    e->akey_tag[entry] = s;
    return 0;
}

// a picture that is no key picture and is decoded into the slot of its stream's
// current key: the second pass of a concealment (host/conceal.c: the concealed
// MBs are zero-vector skip records that name the slot itself, which no other
// picture does) reconstructs the key picture again, now filtered; any other
// picture replaces it
static bool accres_second_pass(const h264mi_engine *e, const MbRec *r, int slot)
{
    for (int m = 0; m < e->nmbs; m++)
        if (r[m].type <= MBT_SKIP && r[m].ref[0] == slot) return true;
    return false;
}

static int accmv_batch(h264mi_engine *e, int npics, const int *stream, const int *cur_slot, const void *const *recs)
{
    accmv_step_args a;
    a.rec = (const uint8_t *)e->d_rec;
    a.w_mbs = e->w; a.W = 16 * e->w; a.H = 16 * e->h; a.nslots = e->nslots;
    for (int k0 = 0; k0 < npics; k0 += ACCMV_STEP_PICS) {
        const int n = npics - k0 < ACCMV_STEP_PICS ? npics - k0 : ACCMV_STEP_PICS;
        memset(a.ref, 0, sizeof(a.ref));
        for (int k = 0; k < ACCMV_STEP_PICS; k++) {
            const int i = k0 + (k < n ? k : 0);
            const size_t b = (size_t)stream[i] * e->nslots;
            a.rec_off[k] = (unsigned long long)i * e->nmbs * sizeof(MbRec);
            a.out[k] = e->d_acc + (b + cur_slot[i]) * acc_words(e);
            a.mode[k] = ACCMV_STEP;
            if (k >= n) continue;
            const MbRec *r = (const MbRec *)recs[i];
            bool key = true;
            for (int m = 0; m < e->nmbs && key; m++) key = r[m].type > MBT_SKIP;
            if (key) {
                e->acc_key[stream[i]]++;
                a.mode[k] = ACCMV_KEY;
            } else {
                for (int s = 0; s < e->nslots; s++)
                    if (s != cur_slot[i] && e->acc_key[stream[i]] && e->acc_ser[b + s] == e->acc_key[stream[i]])
                        a.ref[k][s] = e->d_acc + (b + s) * acc_words(e);
            }
            e->acc_ser[b + cur_slot[i]] = e->acc_key[stream[i]];
            if (!e->d_akey) continue;
            // (a later picture of this batch into the same slot leaves nothing to copy after the launch)
            bool last = true;
            for (int j = i + 1; j < npics && last; j++) last = stream[j] != stream[i] || cur_slot[j] != cur_slot[i];
            if (key) {
                e->akey_slot[stream[i]] = last ? cur_slot[i] : -1;
                if (last && accres_copy_key(e, stream[i], cur_slot[i])) return -1;
            } else if (e->akey_slot[stream[i]] == cur_slot[i]) {
                if (last && accres_second_pass(e, r, cur_slot[i])) {
                    if (accres_copy_key(e, stream[i], cur_slot[i])) return -1;
                } else {
                    e->akey_slot[stream[i]] = -1;
                }
            }
        }
        accmv_step_launch(n, e->st, a);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// coefficient retention (h264mi_engine_keep_coefs): a kept batch holds the
// worst case of every MB -- 16 luma, 8 chroma AC, 1 luma DC and 2 chroma DC
// blocks (I_PCM's 12 fit)
#define KEEP_COEF_MB 27
static size_t keepc_cap(const h264mi_engine *e) { return (size_t)KEEP_COEF_MB * e->nmbs; }

// the same for the uploaded pool: picture i's ncoef[i] blocks, which follow
// those of the pictures before it in d_coef, to the start of its slot's kept
// batch (the records are picture-relative: the kept base is 0).  A picture
// with more blocks than a batch holds is not kept and its slot exports zeros.
static int keep_coef_batch(h264mi_engine *e, int npics, const int *stream, const int *cur_slot, const uint32_t *ncoef)
{
    size_t cbase = 0;
    for (int i = 0; i < npics; cbase += ncoef[i++]) {
        const size_t k = (size_t)stream[i] * e->nslots + cur_slot[i];
        e->keepc_ok[k] = ncoef[i] <= keepc_cap(e);
        if (e->keepc_ok[k] && ncoef[i])
            HIPCHECK(hipMemcpyAsync(e->d_keepc + k * keepc_cap(e) * 16, e->d_coef + cbase * 16, (size_t)ncoef[i] * 32,
                                    hipMemcpyDeviceToDevice, e->st));
    }
    return 0;
}

// intra_heavy: the batch's launch shape hint when the caller knows it (the
// host path counts intra MBs while parsing); -1: derive it from the records

extern "C" int h264mi_engine_decode(h264mi_engine *e, int npics, const int *stream, const int *cur_slot,
                                    const void *const *recs, const int16_t *const *coefs, const uint32_t *ncoef)
{
    return engine_decode_host(e, npics, stream, cur_slot, recs, coefs, ncoef, -1);
}

// the three steps the two upload paths below share
// room for `total` coefficient blocks in the device pool and its pinned staging
static int reserve_coefs(h264mi_engine *e, size_t total)
{
    if (total + 16 <= e->coef_cap) return 0;
    HIPCHECK(hipStreamSynchronize(e->st));
    (void)hipFree(e->d_coef);
    (void)hipHostFree(e->h_coef);
    e->coef_cap = e->h_coef_cap = total + total / 2 + 1024;
    HIPCHECK(hipMalloc(&e->d_coef, e->coef_cap * 32));
    HIPCHECK(hipHostMalloc(&e->h_coef, e->h_coef_cap * 32, hipHostMallocDefault));
    return 0;
}

// batch picture i's descriptor in the pinned staging: its records at
// d_rec + i * nmbs, its coefficient blocks from cbase on; the flags from a
// scan of its records (intra-heavy: more than half its MBs intra; no
// deblocking: no MB filters an inner edge)
static void fill_pic_desc(h264mi_engine *e, int i, int stream, int cur_slot, const void *rec, size_t cbase)
{
    PicDesc &pd = e->h_pics[i];
    pd.rec_base = (uint32_t)(i * e->nmbs);
    pd.frame_base = (uint32_t)(stream * e->nslots);
    pd.cur_slot = (uint32_t)cur_slot;
    const MbRec *r = (const MbRec *)rec;
    int n = 0, db = 0;
    for (int m = 0; m < e->nmbs; m++) { n += r[m].type >= MBT_I4x4; db |= r[m].avail & DB_INNER; }
    pd.flags = (2 * n > e->nmbs ? PD_INTRA_HEAVY : 0) | (db ? 0 : PD_NO_DEBLOCK);
    pd.coef_base = (uint32_t)cbase;
    pd.rsv[0] = pd.rsv[1] = pd.rsv[2] = 0;
}

// what is kept of the uploaded batch, queued behind its launch
static int retain_batch(h264mi_engine *e, int npics, const int *stream, const int *cur_slot, const void *const *recs,
                        const uint32_t *ncoef)
{
    if (e->d_acc && accmv_batch(e, npics, stream, cur_slot, recs)) return -1;
    if (e->d_keep && keep_batch(e, npics, stream, cur_slot)) return -1;
    return e->d_keepc ? keep_coef_batch(e, npics, stream, cur_slot, ncoef) : 0;
}

int engine_decode_host(h264mi_engine *e, int npics, const int *stream, const int *cur_slot,
                       const void *const *recs, const int16_t *const *coefs, const uint32_t *ncoef,
                       int intra_heavy)
{
    if (!e || npics < 1 || npics > e->nstreams) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    // staging buffers are reused: wait until the previous upload consumed them
    HIPCHECK(hipEventSynchronize(e->ev_staged));
    size_t total = 0;
    for (int i = 0; i < npics; i++) total += ncoef[i];
    if (reserve_coefs(e, total)) return -1;
    size_t cbase = 0;
    for (int i = 0; i < npics; i++) {
        if (stream[i] < 0 || stream[i] >= e->nstreams || cur_slot[i] < 0 || cur_slot[i] >= e->nslots) return -1;
        memcpy(e->h_rec + (size_t)i * e->nmbs, recs[i], sizeof(MbRec) * e->nmbs);
        if (ncoef[i]) memcpy(e->h_coef + cbase * 16, coefs[i], (size_t)ncoef[i] * 32);
        fill_pic_desc(e, i, stream[i], cur_slot[i], recs[i], cbase);
        cbase += ncoef[i];
    }
    HIPCHECK(hipMemcpyAsync(e->d_rec, e->h_rec, sizeof(MbRec) * e->nmbs * npics, hipMemcpyHostToDevice, e->st));
    if (cbase) HIPCHECK(hipMemcpyAsync(e->d_coef, e->h_coef, cbase * 32, hipMemcpyHostToDevice, e->st));
    HIPCHECK(hipMemcpyAsync(e->d_pics, e->h_pics, sizeof(PicDesc) * npics, hipMemcpyHostToDevice, e->st));
    HIPCHECK(hipEventRecord(e->ev_staged, e->st));
    // the batch's shape hint from its records (launch_nmc)
    int heavy = intra_heavy > 0;
    for (int i = 0; i < npics && !heavy && intra_heavy < 0; i++) heavy = (e->h_pics[i].flags & PD_INTRA_HEAVY) != 0;
    e->launch_intra = heavy;
    if (launch_batch(e, npics, 1, e->d_rec, e->d_coef, e->d_pics, NULL, NULL, NULL)) return -1;
    return retain_batch(e, npics, stream, cur_slot, recs, ncoef);
}

// one picture whose records and coefficients are already pinned: uploaded
// from where they are, no staging copy
int engine_decode_direct(h264mi_engine *e, int stream, int cur_slot, const void *rec, const int16_t *coef,
                         uint32_t ncoef, int intra_heavy)
{
    if (!e || stream < 0 || stream >= e->nstreams || cur_slot < 0 || cur_slot >= e->nslots) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    // the descriptor staging is reused: wait until the previous upload consumed it
    HIPCHECK(hipEventSynchronize(e->ev_staged));
    if (reserve_coefs(e, ncoef)) return -1;
    fill_pic_desc(e, 0, stream, cur_slot, rec, 0);
    HIPCHECK(hipMemcpyAsync(e->d_rec, rec, sizeof(MbRec) * e->nmbs, hipMemcpyHostToDevice, e->st));
    if (ncoef) HIPCHECK(hipMemcpyAsync(e->d_coef, coef, (size_t)ncoef * 32, hipMemcpyHostToDevice, e->st));
    HIPCHECK(hipMemcpyAsync(e->d_pics, e->h_pics, sizeof(PicDesc), hipMemcpyHostToDevice, e->st));
    HIPCHECK(hipEventRecord(e->ev_staged, e->st));
    e->launch_intra = intra_heavy >= 0 ? intra_heavy : (e->h_pics[0].flags & PD_INTRA_HEAVY) != 0;
    if (launch_batch(e, 1, 1, e->d_rec, e->d_coef, e->d_pics, NULL, NULL, NULL)) return -1;
    return retain_batch(e, 1, &stream, &cur_slot, &rec, &ncoef);
}

int engine_records_wait(h264mi_engine *e)
{
    if (!e) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    HIPCHECK(hipEventSynchronize(e->ev_staged));
    return 0;
}

// the next launch's content, for callers holding their records on the device
// (launch_nmc): 1 = some picture has more than half its MBs intra, 0 = none
extern "C" int h264mi_engine_hint_intra(h264mi_engine *e, int intra_heavy)
{
    if (!e || intra_heavy < 0 || intra_heavy > 1) return -1;
    e->launch_intra = intra_heavy;
    return 0;
}

// the next frame-pipelined launch's dependency mode: 1 whole MB rows, 2 (MB
// row, MB column) cells, 0 the engine's default (H264MI_DEP_MODE)
extern "C" int h264mi_engine_hint_deps(h264mi_engine *e, int mode)
{
    if (!e || mode < 0 || mode > DEP_COLS) return -1;
    e->launch_dep = mode;
    return 0;
}
extern "C" int h264mi_engine_last_deps(h264mi_engine *e) { return e ? e->last_dep : -1; }
extern "C" int h264mi_engine_last_mc_waves(h264mi_engine *e) { return e ? e->last_nmc : -1; }

extern "C" int h264mi_engine_decode_device(h264mi_engine *e, int npics, const void *d_recs, const int16_t *d_coef,
                                           const void *d_pics)
{
    return h264mi_engine_decode_device_next(e, npics, d_recs, d_coef, d_pics, NULL, NULL, NULL);
}

extern "C" int h264mi_engine_decode_device_next(h264mi_engine *e, int npics, const void *d_recs,
                                                const int16_t *d_coef, const void *d_pics, const void *next_recs,
                                                const int16_t *next_coef, const void *next_pics)
{
    if (!e || npics < 1 || npics > e->nstreams || !d_recs || !d_pics) return -1;
    if (next_recs && !next_pics) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    return launch_batch(e, npics, 1, (const MbRec *)d_recs, d_coef, (const PicDesc *)d_pics, (const MbRec *)next_recs,
                        next_coef, (const PicDesc *)next_pics);
}

// frame-pipelined batches: P (<= the engine's steps) consecutive pictures of
// each of S streams in one launch, step-major (descriptor j * S + s), every
// PicDesc.rec_base relative to d_recs; the caller guarantees that no picture
// of the batch writes a slot an earlier picture of the batch reads or writes
extern "C" int h264mi_engine_decode_device_steps(h264mi_engine *e, int S, int P, const void *d_recs,
                                                 const int16_t *d_coef, const void *d_pics, const void *next_recs,
                                                 const int16_t *next_coef, const void *next_pics)
{
    if (!e || S < 1 || S > e->nstreams || P < 1 || P > e->steps || !d_recs || !d_pics) return -1;
    if (next_recs && !next_pics) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    return launch_batch(e, S, P, (const MbRec *)d_recs, d_coef, (const PicDesc *)d_pics, (const MbRec *)next_recs,
                        next_coef, (const PicDesc *)next_pics);
}

// the same, naming the next batch's steps (1 .. the engine's steps) when it
// has a different count: its k_prep in this launch's tail covers S * next_P
// pictures (a plan mixing one- and two-step launches keeps its tail preps)
extern "C" int h264mi_engine_decode_device_steps_next(h264mi_engine *e, int S, int P, const void *d_recs,
                                                      const int16_t *d_coef, const void *d_pics,
                                                      const void *next_recs, const int16_t *next_coef,
                                                      const void *next_pics, int next_P)
{
    if (!e || S < 1 || S > e->nstreams || P < 1 || P > e->steps || !d_recs || !d_pics) return -1;
    if (!next_recs || !next_pics || next_P < 1 || next_P > e->steps) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    return launch_batch(e, S, P, (const MbRec *)d_recs, d_coef, (const PicDesc *)d_pics, (const MbRec *)next_recs,
                        next_coef, (const PicDesc *)next_pics, S * next_P);
}

// diagnostics: resident k_wgpp workgroups per CU the runtime computes for
// the main single-row kernel (rpw 1), and its kernel attributes
extern "C" int h264mi_kernel_occupancy(int *blocks_per_cu, int *lds_bytes, int *vgprs, int *sgprs)
{
    constexpr int vi = wgpp_find(3, false, 1, false, DEP_NONE);
    static_assert(vi >= 0, "the main single-row instance is in WGPP_VARIANTS");
    const WgppLaunch &k = wgpp_launch[vi];
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, k.fn) != hipSuccess) return -1;
    int n = 0;
    const size_t lds = k.lds(120, false);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k.fn, wgpp_block_size(wgpp_variants[vi].nmc, wgpp_variants[vi].rpw), lds) != hipSuccess) return -1;
    if (blocks_per_cu) *blocks_per_cu = n;
    if (lds_bytes) *lds_bytes = (int)(fa.sharedSizeBytes + lds);
    if (vgprs) *vgprs = fa.numRegs;
    if (sgprs) *sgprs = 0;
    return 0;
}

// the profiling kernels' stamp buffer, sized for the engine's current
// picture capacity (every picture of a launch: per-row and per-MB stamps)
static int prof_alloc(h264mi_engine *e)
{
    (void)hipFree(e->d_prof);
    e->d_prof = NULL;
    e->prof_cap = (size_t)e->pipe_cap * e->h * PROF_ROW + (size_t)e->pipe_cap * e->nmbs * PROF_MB;
    HIPCHECK(hipMalloc(&e->d_prof, sizeof(unsigned long long) * e->prof_cap));
    HIPCHECK(hipMemset(e->d_prof, 0, sizeof(unsigned long long) * e->prof_cap));
    return 0;
}

extern "C" int h264mi_engine_set_steps(h264mi_engine *e, int steps)
{
    // (frame-pipelined launches name the earlier steps' target slots in a
    // 32-bit mask: recon_kernels.hip dep_wait)
    // (a later step's producers: by slot equality, 8-bit slots (DEP_COLS), or
    // a 32-bit slot mask (DEP_ROWS; engines of more slots run DEP_COLS))
    if (!e || steps < 1 || steps > H264MI_MAX_STEPS || (steps > 1 && e->nslots > 255)) return -1;
    if (steps == e->steps) return 0;
    if (h264mi_engine_sync(e)) return -1;
    free_pic_buffers(e);
    if (alloc_pic_buffers(e, e->nstreams * steps)) return -1;
    e->steps = steps;
    e->prepped_rec = NULL; e->prepped_pics = NULL;
    e->prep_parity = 0;
    // a profiling buffer allocated for the old capacity would be overrun by
    // the stamps of a launch of more pictures: resize it with the capacity
    if (e->d_prof && prof_alloc(e)) return -1;
    HIPCHECK(hipStreamSynchronize(e->st));
    return 0;
}

extern "C" const char *h264mi_engine_kernel(h264mi_engine *e)
{
    return e && e->last_kernel ? e->last_kernel : "";
}

// wait for everything queued on the engine's stream (sleeping under
// H264MI_BLOCKING_SYNC); no flag accounting
int engine_wait(h264mi_engine *e)
{
    HIPCHECK(hipSetDevice(e->dev));
    if (e->ev_block) {
        HIPCHECK(hipEventRecord(e->ev_block, e->st));
        HIPCHECK(hipEventSynchronize(e->ev_block));
    } else {
        HIPCHECK(hipStreamSynchronize(e->st));
    }
    return 0;
}

extern "C" int h264mi_engine_sync(h264mi_engine *e)
{
    if (!e) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    // per-picture error flags OR-accumulate over every launch since the last
    // sync (no per-launch reset): fetch them into pinned memory and clear
    // them behind the launches, one wait for all, then count the flagged
    // picture slots
    HIPCHECK(hipMemcpyAsync(e->h_err, e->d_err, sizeof(unsigned) * e->pipe_cap, hipMemcpyDeviceToHost, e->st));
    HIPCHECK(hipMemsetAsync(e->d_err, 0, sizeof(unsigned) * e->pipe_cap, e->st));
    // a blocking-sync event: the waiting thread sleeps whatever the device's
    // scheduling flags (which take effect only before the first context)
    if (engine_wait(e)) return -1;
    for (int i = 0; i < e->pipe_cap; i++) {
        e->err_accum += e->h_err[i] ? 1 : 0;
        e->err_bits |= e->h_err[i];
    }
    return 0;
}

extern "C" int h264mi_engine_rows_per_workgroup(h264mi_engine *e, int npics)
{
    return e && npics > 0 ? rows_per_wg(e, npics) : 0;
}

extern "C" uint32_t h264mi_engine_errors(h264mi_engine *e)
{
    if (!e) return 0;
    uint32_t v = e->err_accum;
    e->err_accum = 0;
    return v;
}

extern "C" uint32_t h264mi_engine_error_bits(h264mi_engine *e)
{
    if (!e) return 0;
    const uint32_t v = e->err_bits;
    e->err_bits = 0;
    return v;
}

extern "C" int h264mi_engine_last_timing(h264mi_engine *e, float *us2)
{
    if (!e || !e->timing) return -1;
    float ms0 = 0, ms1 = 0;
    HIPCHECK(hipEventSynchronize(e->ev2));
    HIPCHECK(hipEventElapsedTime(&ms1, e->ev0, e->ev2));
    us2[0] = ms0 * 1000.f;
    us2[1] = ms1 * 1000.f;
    return 0;
}

extern "C" int h264mi_engine_set_timing(h264mi_engine *e, int max_batches)
{
    if (!e) return -1;
    if (e->tev) {
        for (int i = 0; i < 3 * e->tev_cap; i++) (void)hipEventDestroy(e->tev[i]);
        free(e->tev);
        e->tev = NULL;
    }
    e->tev_cap = e->tev_n = 0;
    e->tev_seq = 0;
    if (max_batches <= 0) return 0;
    e->tev = (hipEvent_t *)calloc((size_t)max_batches * 3, sizeof(hipEvent_t));
    if (!e->tev) return -1;
    for (int i = 0; i < 3 * max_batches; i++) HIPCHECK(hipEventCreate(&e->tev[i]));
    e->tev_cap = max_batches;
    return 0;
}

extern "C" int h264mi_engine_set_timing_stride(h264mi_engine *e, int stride)
{
    if (!e || stride < 1) return -1;
    e->tev_stride = stride;
    e->tev_seq = 0;
    return 0;
}

extern "C" int h264mi_engine_timing_list(h264mi_engine *e, double *us, int cap)
{
    if (!e || !e->tev || !us || cap < 0) return -1;
    if (h264mi_engine_sync(e)) return -1;
    const int n = e->tev_n < cap ? e->tev_n : cap;
    for (int i = 0; i < n; i++) {
        float m = 0;
        HIPCHECK(hipEventElapsedTime(&m, e->tev[3 * i], e->tev[3 * i + 2]));
        us[i] = m * 1000.0;
    }
    return n;
}

extern "C" int h264mi_engine_timing_report(h264mi_engine *e, double *inter_us, double *wave_us, int *nbatches)
{
    if (!e || !e->tev) return -1;
    if (h264mi_engine_sync(e)) return -1;
    double a = 0, b = 0;
    for (int i = 0; i < e->tev_n; i++) {
        float m0 = 0, m1 = 0;
        HIPCHECK(hipEventElapsedTime(&m1, e->tev[3 * i], e->tev[3 * i + 2]));
        a += m0 * 1000.0;
        b += m1 * 1000.0;
    }
    *inter_us = a;
    *wave_us = b;
    *nbatches = e->tev_n;
    e->tev_n = 0;
    return 0;
}

extern "C" int h264mi_engine_profile(h264mi_engine *e, int enable, unsigned long long *out, size_t n)
{
    if (!e) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    if (out && e->d_prof) {
        HIPCHECK(hipStreamSynchronize(e->st));
        HIPCHECK(hipMemcpy(out, e->d_prof, sizeof(unsigned long long) * (n < e->prof_cap ? n : e->prof_cap),
                           hipMemcpyDeviceToHost));
    }
    if (enable && !e->d_prof) {
        if (prof_alloc(e)) return -1;
    } else if (!enable && e->d_prof) {
        HIPCHECK(hipStreamSynchronize(e->st));
        (void)hipFree(e->d_prof);
        e->d_prof = NULL;
        e->prof_cap = 0;
    }
    return 0;
}

// D2H of a slot as packed I420 on `st`, asynchronous: the luma plane and the
// padded chroma rows (H264MI_CPITCH) as one strided copy of 2 * h * 8 rows
int engine_copy_out(h264mi_engine *e, int stream, int slot, uint8_t *dst, hipStream_t st)
{
    const uint8_t *src = e->d_frames + e->frame_bytes * ((size_t)stream * e->nslots + slot);
    const size_t ysz = (size_t)e->nmbs * 256, cw = (size_t)e->w * 8;
    if ((size_t)e->cpitch == cw) {
        HIPCHECK(hipMemcpyAsync(dst, src, e->pic_bytes, hipMemcpyDeviceToHost, st));
        return 0;
    }
    HIPCHECK(hipMemcpyAsync(dst, src, ysz, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpy2DAsync(dst + ysz, cw, src + ysz, (size_t)e->cpitch, cw, (size_t)e->h * 16, hipMemcpyDeviceToHost, st));
    return 0;
}
size_t engine_slot_bytes(const h264mi_engine *e) { return e->frame_bytes; }

extern "C" int h264mi_engine_read(h264mi_engine *e, int stream, int slot, uint8_t *dst)
{
    if (!e || stream < 0 || stream >= e->nstreams || slot < 0 || slot >= e->nslots) return -1;
    if (h264mi_engine_sync(e)) return -1;
    if (engine_copy_out(e, stream, slot, dst, e->st)) return -1;
    HIPCHECK(hipStreamSynchronize(e->st));
    return 0;
}

// I420 -> RGBA (DecoderPost.js `rgb: true`, color.hip) for `npics` pictures
// of width x height pixels at in + k * in_stride -> out + k * out_stride,
// device pointers, on `stream` (NULL: the null stream); asynchronous
extern "C" int h264mi_yuv2rgba_device_pitch(const void *d_i420, void *d_rgba, int width, int height, int cpitch,
                                            int npics, size_t in_stride, size_t out_stride, void *stream)
{
    if (!d_i420 || !d_rgba || width <= 0 || height <= 0 || (width & 15) || (height & 15) || npics < 1 ||
        cpitch < width / 2)
        return -1;
    const int nblk = ((height >> 1) * (width >> 2) + 127) >> 7;
    hipLaunchKernelGGL(k_yuv2rgba, dim3(nblk, npics), dim3(64), 0, (hipStream_t)stream,
                       (const uint8_t *)d_i420, (uint8_t *)d_rgba, width, height, cpitch, in_stride, out_stride);
    HIPCHECK(hipGetLastError());
    return 0;
}

extern "C" int h264mi_yuv2rgba_device(const void *d_i420, void *d_rgba, int width, int height, int npics,
                                      size_t in_stride, size_t out_stride, void *stream)
{
    return h264mi_yuv2rgba_device_pitch(d_i420, d_rgba, width, height, width / 2, npics, in_stride, out_stride, stream);
}

extern "C" int h264mi_engine_read_rgba(h264mi_engine *e, int stream, int slot, uint8_t *dst)
{
    if (!e || stream < 0 || stream >= e->nstreams || slot < 0 || slot >= e->nslots) return -1;
    const size_t bytes = (size_t)e->nmbs * 256 * 4;
    if (!e->d_rgba) HIPCHECK(hipMalloc(&e->d_rgba, bytes));
    if (h264mi_yuv2rgba_device_pitch(e->d_frames + e->frame_bytes * ((size_t)stream * e->nslots + slot), e->d_rgba,
                                     e->w * 16, e->h * 16, e->cpitch, 1, 0, 0, e->st))
        return -1;
    HIPCHECK(hipMemcpyAsync(dst, e->d_rgba, bytes, hipMemcpyDeviceToHost, e->st));
    HIPCHECK(hipStreamSynchronize(e->st));
    return 0;
}

// The crop window (x, y, cw, ch; all even, inside the picture) of `npics`
// pictures of width x height pixels, chroma rows cpitch bytes apart, at
// d_in + k * in_stride -> packed at d_out + k * out_stride: I420 in the layout
// of the reference testbench's CropPicture, or RGBA (crop.hip); device
// pointers, asynchronous on `stream`.  RGBA output is 8-byte aligned.
// -1 (nothing launched) on a bad argument.
extern "C" int h264mi_crop_device_pitch(const void *d_in, void *d_out, int width, int height, int cpitch, int x, int y,
                                        int cw, int ch, int rgba, int npics, size_t in_stride, size_t out_stride,
                                        void *stream)
{
    if (!d_in || !d_out || width <= 0 || height <= 0 || ((width | height) & 1) || npics < 1 || cpitch < width / 2 ||
        x < 0 || y < 0 || cw <= 0 || ch <= 0 || ((x | y | cw | ch) & 1) || cw > width - x || ch > height - y)
        return -1;
    const uint8_t *in = (const uint8_t *)d_in;
    uint8_t *out = (uint8_t *)d_out;
    if (rgba) {
        const size_t al = (size_t)(uintptr_t)out | (npics > 1 ? out_stride : 0);
        if (al & 7) return -1;
        const int nblk = ((ch >> 1) * ((cw + 3) >> 2) + 127) >> 7;
        if (!(cw & 3) && !(al & 15))
            hipLaunchKernelGGL(k_crop_rgba<true>, dim3(nblk, npics), dim3(64), 0, (hipStream_t)stream, in, out, width,
                               height, cpitch, x, y, cw, ch, in_stride, out_stride);
        else
            hipLaunchKernelGGL(k_crop_rgba<false>, dim3(nblk, npics), dim3(64), 0, (hipStream_t)stream, in, out, width,
                               height, cpitch, x, y, cw, ch, in_stride, out_stride);
    } else {
        // the most chunks the three planes can cover, whatever the output's alignment
        const int ny = cw * ch, nc = (cw >> 1) * (ch >> 1);
        const int chunks = ((ny + 30) >> 4) + 2 * ((nc + 30) >> 4);
        hipLaunchKernelGGL(k_crop_i420, dim3((chunks + 127) >> 7, npics), dim3(64), 0, (hipStream_t)stream, in, out,
                           width, height, cpitch, x, y, cw, ch, in_stride, out_stride);
    }
    HIPCHECK(hipGetLastError());
    return 0;
}

// D2H of the crop window of a slot, packed I420 or RGBA (h264mi_crop_device_pitch
// into a staging buffer, one contiguous copy); syncs the engine first
extern "C" int h264mi_engine_read_crop(h264mi_engine *e, int stream, int slot, int x, int y, int cw, int ch, int rgba,
                                       uint8_t *dst)
{
    if (!e || !dst || stream < 0 || stream >= e->nstreams || slot < 0 || slot >= e->nslots) return -1;
    const int width = e->w * 16, height = e->h * 16;
    if (x < 0 || y < 0 || cw <= 0 || ch <= 0 || ((x | y | cw | ch) & 1) || cw > width - x || ch > height - y) return -1;
    if (h264mi_engine_sync(e)) return -1;
    const uint8_t *src = e->d_frames + e->frame_bytes * ((size_t)stream * e->nslots + slot);
    const size_t bytes = rgba ? (size_t)cw * ch * 4 : (size_t)cw * ch * 3 / 2;
    if (!e->d_rgba) HIPCHECK(hipMalloc(&e->d_rgba, (size_t)e->nmbs * 256 * 4));
    if (h264mi_crop_device_pitch(src, e->d_rgba, width, height, e->cpitch, x, y, cw, ch, rgba, 1, 0, 0, e->st)) return -1;
    HIPCHECK(hipMemcpyAsync(dst, e->d_rgba, bytes, hipMemcpyDeviceToHost, e->st));
    HIPCHECK(hipStreamSynchronize(e->st));
    return 0;
}

// a mode the engine-level exports accept: RGB with a colour id 0..3 (bits 12
// and 13 mean nothing without STREAM, which needs a stream: refused) or GRAY
// with no colour bits, and no bit from 14 up
static bool tensor_mode_ok(int mode)
{
    if (mode & ~0x3FFF) return false;
    if (H264MI_TENSOR_LAYOUT(mode) == H264MI_TENSOR_GRAY) return mode == H264MI_TENSOR_GRAY;
    return H264MI_TENSOR_LAYOUT(mode) == H264MI_TENSOR_RGB && H264MI_TENSOR_COLOUR(mode) < TENSOR_COLOUR_SETS;
}

// a window / mode / dtype a tensor export accepts (the window rules are
// h264mi_crop_device_pitch's)
static bool tensor_desc_ok(const h264mi_tensor_desc *t, int width, int height)
{
    return t && tensor_mode_ok(t->mode) && tensor_desc_fixed_ok(t) && tensor_window_ok(t, width, height);
}

extern "C" int h264mi_tensor_colour_coeffs(int id, int out[6])
{
    if (id < 0 || id >= TENSOR_COLOUR_SETS || !out) return -1;
    const colour_set &c = tensor_colour_sets[id];
    out[0] = c.ky; out[1] = c.k0; out[2] = c.crv; out[3] = c.cgu; out[4] = c.cgv; out[5] = c.cbu;
    return 0;
}

// a resize descriptor h264mi_tensor_resize_device_pitch accepts
static bool resize_desc_ok(const h264mi_tensor_resize_desc *d, int width, int height)
{
    return d && tensor_mode_ok(d->t.mode) && resize_desc_fixed_ok(d) && resize_window_ok(d, width, height);
}

// a field descriptor h264mi_mbinfo_device accepts on a w_mbs x h_mbs picture
static bool mbinfo_desc_ok(const h264mi_mbinfo_desc *d, int w_mbs, int h_mbs)
{
    return d && mbinfo_desc_fixed_ok(d) && mbinfo_window_ok(d, w_mbs, h_mbs);
}

// a residual descriptor h264mi_residual_device accepts on a w_mbs x h_mbs picture
static bool residual_desc_ok(const h264mi_residual_desc *d, int w_mbs, int h_mbs)
{
    return d && residual_desc_fixed_ok(d) && residual_window_ok(d, w_mbs, h_mbs);
}

#define EXPORT_MAX_PICS TENSOR_MAX_PICS
static_assert(MBINFO_MAX_PICS == EXPORT_MAX_PICS && RESID_MAX_PICS == EXPORT_MAX_PICS,
              "every export kernel takes the same number of pictures per launch");
static_assert(H264MI_RESIZE_MAX_DIM == RESIZE_MAX_DIM, "common/export_desc.h and resize.hip name the same bound");
static_assert(export_elem_size(H264MI_TENSOR_U8) == tensor_elem_size(TENSOR_U8) &&
                  export_elem_size(H264MI_TENSOR_F16) == tensor_elem_size(TENSOR_F16) &&
                  export_elem_size(H264MI_TENSOR_BF16) == tensor_elem_size(TENSOR_BF16) &&
                  export_elem_size(H264MI_TENSOR_F32) == tensor_elem_size(TENSOR_F32) &&
                  export_elem_size(H264MI_TENSOR_I16) == tensor_elem_size(TENSOR_I16),
              "common/export_desc.h and tensor.hip give the element types the same sizes");

// the kernels may store 16 bytes at a time: every row of row_bytes bytes of
// every picture (out_stride apart) starts on a multiple of 16
static bool export_v16(const void *d_out, size_t out_stride, size_t row_bytes)
{
    return !(((size_t)(uintptr_t)d_out | out_stride | row_bytes) & 15);
}

// The launches of a *_device entry point over npics pictures, at most
// EXPORT_MAX_PICS each: a launch's offsets into a_off, zero-padded, and its
// first picture's address into *a_out, then launch(k0, n) for the n pictures
// from k0 on.
template <class Launch>
static int export_launches(int npics, const size_t *offsets, unsigned long long *a_off, uint8_t **a_out, void *d_out,
                           size_t out_stride, Launch launch)
{
    for (int k0 = 0; k0 < npics; k0 += EXPORT_MAX_PICS) {
        const int n = npics - k0 < EXPORT_MAX_PICS ? npics - k0 : EXPORT_MAX_PICS;
        for (int k = 0; k < EXPORT_MAX_PICS; k++) a_off[k] = k < n ? offsets[k0 + k] : 0;
        *a_out = (uint8_t *)d_out + (size_t)k0 * out_stride;
        launch(k0, n);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// Both tensor exports (r != NULL: resized, t = &r->t): one check and one fill
// of what their kernels share, resize_args::t
static int tensor_device(const void *d_in, const size_t *in_offsets, int npics, int width, int height, int cpitch,
                         const h264mi_tensor_desc *t, const h264mi_tensor_resize_desc *r, void *d_out,
                         size_t out_stride, hipStream_t stream)
{
    static_assert(H264MI_TENSOR_RGB == TENSOR_RGB && H264MI_TENSOR_GRAY == TENSOR_GRAY &&
                      H264MI_TENSOR_U8 == TENSOR_U8 && H264MI_TENSOR_F16 == TENSOR_F16 &&
                      H264MI_TENSOR_BF16 == TENSOR_BF16 && H264MI_TENSOR_F32 == TENSOR_F32 &&
                      H264MI_TENSOR_COLOUR_BT709_FULL == TENSOR_COLOUR_SETS - 1,
                  "include/h264mi.h and tensor.hip name the same modes, element types and colour sets");
    if (!d_in || !in_offsets || !d_out || width <= 0 || height <= 0 || ((width | height) & 1) || npics < 1 ||
        cpitch < width / 2 || (r ? !resize_desc_ok(r, width, height) : !tensor_desc_ok(t, width, height)))
        return -1;
    const size_t es = export_elem_size(t->dtype);
    if (!export_aligned(d_out, out_stride, es)) return -1;
    const bool v16 = export_v16(d_out, out_stride, (size_t)t->cw * es);
    const int layout = H264MI_TENSOR_LAYOUT(t->mode), colour = H264MI_TENSOR_COLOUR(t->mode);
    resize_args ra;
    tensor_args &a = ra.t;
    a.in = (const uint8_t *)d_in;
    a.width = width; a.height = height; a.cpitch = cpitch;
    a.x = t->x; a.y = t->y; a.cw = t->cw; a.ch = t->ch;
    a.out_stride = out_stride;
    for (int p = 0; p < 3; p++) { a.scale[p] = t->scale[p]; a.bias[p] = t->bias[p]; }
    a.col = tensor_colour_sets[colour];     // (set 0 runs the kernels with the reference's literals)
    if (r) { ra.ow = r->ow; ra.oh = r->oh; }
    return export_launches(npics, in_offsets, a.in_off, &a.out, d_out, out_stride, [&](int, int n) {
        if (r) resize_launch(layout, t->dtype, colour != 0, n, stream, ra);
        else tensor_launch(layout, t->dtype, v16, colour != 0, n, stream, a);
    });
}

// Pictures as planar tensors (tensor.hip): the window desc->(x, y, cw, ch) of
// the npics pictures of width x height pixels that start in_offsets[k] bytes
// after d_in (chroma rows cpitch bytes apart), as contiguous (planes, ch, cw)
// elements of desc->dtype at d_out + k * out_stride; device pointers,
// asynchronous on `stream`; TENSOR_MAX_PICS pictures per launch.  -1 (nothing
// launched) on a bad argument.
extern "C" int h264mi_tensor_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width, int height,
                                          int cpitch, const h264mi_tensor_desc *desc, void *d_out, size_t out_stride,
                                          void *stream)
{
    return tensor_device(d_in, in_offsets, npics, width, height, cpitch, desc, NULL, d_out, out_stride, (hipStream_t)stream);
}

// The same pictures resized (resize.hip): the window filtered to desc->oh x
// desc->ow samples per plane, picture k's (planes, oh, ow) elements at d_out +
// k * out_stride.  1 <= ow, oh <= 16384 and, per axis, at most 32 source
// samples per output (64 taps); filter = H264MI_RESIZE_TRIANGLE.  Stateless:
// the tap tables are made in the kernel.  -1 (nothing launched) on a bad
// argument.
extern "C" int h264mi_tensor_resize_device_pitch(const void *d_in, const size_t *in_offsets, int npics, int width,
                                                 int height, int cpitch, const h264mi_tensor_resize_desc *desc,
                                                 void *d_out, size_t out_stride, void *stream)
{
    return tensor_device(d_in, in_offsets, npics, width, height, cpitch, desc ? &desc->t : NULL, desc, d_out, out_stride,
                         (hipStream_t)stream);
}

// An export of the slots (streams[k], slots[k]), k < n, into the caller's
// device memory with no host synchronisation: the engine's stream waits for
// what `stream` (NULL: the null stream; ours is non-blocking, so that too goes
// through events) holds already -- d_out may have been recycled on it --,
// launch() queues the kernels on the engine's stream, behind every launch
// queued so far and ahead of every later one, and `stream` waits for them.
// es: the element size d_out and out_stride are multiples of.
template <class Launch>
static int export_ordered(h264mi_engine *e, int n, const int *streams, const int *slots, void *d_out, size_t out_stride,
                          size_t es, void *stream, Launch launch)
{
    for (int k = 0; k < n; k++)
        if (streams[k] < 0 || streams[k] >= e->nstreams || slots[k] < 0 || slots[k] >= e->nslots) return -1;
    if (!export_aligned(d_out, out_stride, es)) return -1;
    if (h264mi_pointer_device(d_out) != e->dev) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    if (!e->ev_exp_in) HIPCHECK(hipEventCreateWithFlags(&e->ev_exp_in, hipEventDisableTiming));
    if (!e->ev_exp_out) HIPCHECK(hipEventCreateWithFlags(&e->ev_exp_out, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(e->ev_exp_in, (hipStream_t)stream));
    HIPCHECK(hipStreamWaitEvent(e->st, e->ev_exp_in, 0));
    const int rc = launch();
    // (also after a failed launch: whatever reached our stream stays ordered)
    HIPCHECK(hipEventRecord(e->ev_exp_out, e->st));
    HIPCHECK(hipStreamWaitEvent((hipStream_t)stream, e->ev_exp_out, 0));
    return rc;
}

// the frame slots as tensors (rdesc != NULL: resized, desc = &rdesc->t)
static int engine_export(h264mi_engine *e, int n, const int *streams, const int *slots, const h264mi_tensor_desc *desc,
                         const h264mi_tensor_resize_desc *rdesc, void *d_out, size_t out_stride, void *stream)
{
    if (!e || n < 1 || !streams || !slots || !d_out) return -1;
    const int width = e->w * 16, height = e->h * 16;
    if (rdesc ? !resize_desc_ok(rdesc, width, height) : !tensor_desc_ok(desc, width, height)) return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->dtype), stream, [&] {
        std::vector<size_t> off((size_t)n);
        for (int k = 0; k < n; k++) off[k] = e->frame_bytes * ((size_t)streams[k] * e->nslots + slots[k]);
        return tensor_device(e->d_frames, off.data(), n, width, height, e->cpitch, desc, rdesc, d_out, out_stride, e->st);
    });
}

extern "C" int h264mi_engine_export_tensor(h264mi_engine *e, int n, const int *streams, const int *slots,
                                           const h264mi_tensor_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    return engine_export(e, n, streams, slots, desc, NULL, d_out, out_stride, stream);
}

// the same, resized (h264mi_tensor_resize_device_pitch)
extern "C" int h264mi_engine_export_tensor_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                   const h264mi_tensor_resize_desc *desc, void *d_out,
                                                   size_t out_stride, void *stream)
{
    return engine_export(e, n, streams, slots, desc ? &desc->t : NULL, desc, d_out, out_stride, stream);
}

// Motion vectors and MB side information as planar fields (mbinfo.hip): the
// window desc->(bx, by, bw, bh) of the 4x4-block grid of the npics record
// batches (w_mbs * h_mbs MbRec each) that start rec_offsets[k] bytes after
// d_recs, as contiguous (nch, bh, bw) elements of desc->dtype at d_out + k *
// out_stride; device pointers, asynchronous on `stream`; MBINFO_MAX_PICS
// pictures per launch.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_mbinfo_device(const void *d_recs, const size_t *rec_offsets, int npics, int w_mbs, int h_mbs,
                                    const h264mi_mbinfo_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    static_assert(H264MI_TENSOR_I16 == TENSOR_I16 && H264MI_MBINFO_MAX_CH == MBINFO_MAX_CH &&
                      H264MI_MBINFO_NCHANNELS == MBI_NCHANNELS && H264MI_MBINFO_MVX == MBI_MVX &&
                      H264MI_MBINFO_MVY == MBI_MVY && H264MI_MBINFO_REF_IDX == MBI_REF_IDX &&
                      H264MI_MBINFO_REF_SLOT == MBI_REF_SLOT && H264MI_MBINFO_MB_TYPE == MBI_MB_TYPE &&
                      H264MI_MBINFO_QP == MBI_QP && H264MI_MBINFO_INTRA_MODE == MBI_INTRA_MODE &&
                      H264MI_MBINFO_CODED == MBI_CODED && H264MI_MBINFO_SLICE == MBI_SLICE,
                  "include/h264mi.h and mbinfo.hip name the same channels and element types");
    if (!d_recs || !rec_offsets || !d_out || npics < 1 || w_mbs < 1 || h_mbs < 1 || w_mbs > 65535 || h_mbs > 65535 ||
        ((size_t)(uintptr_t)d_recs & 15) || !mbinfo_desc_ok(desc, w_mbs, h_mbs))
        return -1;
    for (int k = 0; k < npics; k++)
        if (rec_offsets[k] % sizeof(MbRec)) return -1;
    const size_t es = export_elem_size(desc->dtype);
    if (!export_aligned(d_out, out_stride, es)) return -1;
    const bool v16 = export_v16(d_out, out_stride, (size_t)desc->bw * es);
    mbinfo_args a;
    a.rec = (const uint8_t *)d_recs;
    a.w_mbs = w_mbs;
    a.bx = desc->bx; a.by = desc->by; a.bw = desc->bw; a.bh = desc->bh; a.nch = desc->nch;
    a.out_stride = out_stride;
    for (int c = 0; c < MBINFO_MAX_CH; c++) {
        a.ch[c] = c < desc->nch ? (uint8_t)desc->ch[c] : 0;
        a.scale[c] = c < desc->nch ? desc->scale[c] : 0.0f;
        a.bias[c] = c < desc->nch ? desc->bias[c] : 0.0f;
    }
    return export_launches(npics, rec_offsets, a.off, &a.out, d_out, out_stride,
                           [&](int, int n) { mbinfo_launch(desc->dtype, v16, n, (hipStream_t)stream, a); });
}

// Record retention: one batch per (stream, slot), 0xFF-filled ("no
// information") until a reconstruction into the slot copies its records there
// (keep_batch).  Off waits for the engine's stream (exports run on it) and frees.
// (One batch more than the slots: it is never copied into, and
// h264mi_engine_export_residual reads it for a slot whose coefficients it does
// not hold.)  keep_hold is the switch itself; the records are held while the
// caller's switch or coefficient retention is on.
static int keep_hold(h264mi_engine *e, int on)
{
    if ((on != 0) == (e->d_keep != NULL)) return 0;
    HIPCHECK(hipSetDevice(e->dev));
    const size_t bytes = sizeof(MbRec) * e->nmbs * ((size_t)e->nslots * e->nstreams + 1);
    if (on) {
        HIPCHECK(hipMalloc(&e->d_keep, bytes));
        if (hipMemsetAsync(e->d_keep, 0xFF, bytes, e->st) != hipSuccess) {
            (void)hipFree(e->d_keep);
            e->d_keep = NULL;
            return -1;
        }
        return 0;
    }
    HIPCHECK(hipStreamSynchronize(e->st));
    (void)hipFree(e->d_keep);
    e->d_keep = NULL;
    return 0;
}

extern "C" int h264mi_engine_keep_records(h264mi_engine *e, int on)
{
    if (!e) return -1;
    e->keep_rec = on != 0;
    return keep_hold(e, e->keep_rec || e->d_keepc);
}

// Coefficient retention: one worst-case batch per (stream, slot), filled by
// keep_coef_batch; it holds the records as well while it is on.  A slot's
// blocks count only with the records of the same reconstruction, so switching
// on starts with no slot valid.  Off waits for the engine's stream and frees.
extern "C" int h264mi_engine_keep_coefs(h264mi_engine *e, int on)
{
    if (!e) return -1;
    if ((on != 0) == (e->d_keepc != NULL)) return 0;
    HIPCHECK(hipSetDevice(e->dev));
    if (on) {
        const size_t nb = (size_t)e->nslots * e->nstreams;
        if (keep_hold(e, 1)) return -1;
        e->keepc_ok = (uint8_t *)calloc(nb, 1);
        if (!e->keepc_ok || hipMalloc(&e->d_keepc, nb * keepc_cap(e) * 32) != hipSuccess) {
            free(e->keepc_ok);
            e->keepc_ok = NULL;
            e->d_keepc = NULL;
            (void)keep_hold(e, e->keep_rec);
            return -1;
        }
        return 0;
    }
    HIPCHECK(hipStreamSynchronize(e->st));
    (void)hipFree(e->d_keepc);
    free(e->keepc_ok);
    e->d_keepc = NULL;
    e->keepc_ok = NULL;
    return keep_hold(e, e->keep_rec);
}

extern "C" int h264mi_engine_forget_records(h264mi_engine *e, int stream, int slot)
{
    if (!e || (!e->d_keep && !e->d_acc) || stream < 0 || stream >= e->nstreams || slot < 0 || slot >= e->nslots)
        return -1;
    HIPCHECK(hipSetDevice(e->dev));
    if (e->keepc_ok) e->keepc_ok[(size_t)stream * e->nslots + slot] = 0;
    if (e->d_keep)
        HIPCHECK(hipMemsetAsync(e->d_keep + ((size_t)stream * e->nslots + slot) * e->nmbs, 0xFF, sizeof(MbRec) * e->nmbs, e->st));
    if (e->d_acc) {
        // the slot's map says nothing about its picture: none as a reference, (x, y, 0) when exported
        e->acc_ser[(size_t)stream * e->nslots + slot] = 0;
        if (e->akey_slot && e->akey_slot[stream] == slot) e->akey_slot[stream] = -1;    // (its entry stays: the GOP's pictures export against it)
        return accmv_clear(e, (size_t)stream * e->nslots + slot, 1);
    }
    return 0;
}

// The kept batches of the slots (streams[k], slots[k]) as fields in the
// caller's memory, ordered between the caller's stream and ours by export_ordered
extern "C" int h264mi_engine_export_mbinfo(h264mi_engine *e, int n, const int *streams, const int *slots,
                                           const h264mi_mbinfo_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    if (!e || !e->d_keep || n < 1 || !streams || !slots || !d_out || !mbinfo_desc_ok(desc, e->w, e->h)) return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->dtype), stream, [&] {
        std::vector<size_t> off((size_t)n);
        for (int k = 0; k < n; k++) off[k] = sizeof(MbRec) * e->nmbs * ((size_t)streams[k] * e->nslots + slots[k]);
        return h264mi_mbinfo_device(e->d_keep, off.data(), n, e->w, e->h, desc, d_out, out_stride, e->st);
    });
}

// The decoded residual as planar tensors (residual.hip): the window desc->(x,
// y, cw, ch), in luma samples of the MB-aligned picture, of the npics pictures
// whose record batches (w_mbs * h_mbs MbRec each) start rec_offsets[k] bytes
// after d_recs and whose coefficient blocks start coef_bases[k] blocks after
// d_coef, a pool of coef_blocks blocks; picture k's planes, contiguous, at
// d_out + k * out_stride; device pointers, asynchronous on `stream`;
// RESID_MAX_PICS pictures per launch.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_residual_device(const void *d_recs, const size_t *rec_offsets, const void *d_coef,
                                      const uint32_t *coef_bases, size_t coef_blocks, int npics, int w_mbs, int h_mbs,
                                      const h264mi_residual_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    static_assert(H264MI_RESID_Y == RESID_Y && H264MI_RESID_UV == RESID_UV && H264MI_RESID_YUV == RESID_YUV,
                  "include/h264mi.h and residual.hip name the same planes");
    if (!d_recs || !rec_offsets || !d_coef || !coef_bases || !d_out || npics < 1 || w_mbs < 1 || h_mbs < 1 ||
        w_mbs > 65535 || h_mbs > 65535 || (((size_t)(uintptr_t)d_recs | (size_t)(uintptr_t)d_coef) & 15) ||
        !residual_desc_ok(desc, w_mbs, h_mbs))
        return -1;
    for (int k = 0; k < npics; k++)
        if (rec_offsets[k] % sizeof(MbRec)) return -1;
    const size_t es = export_elem_size(desc->dtype);
    if (!export_aligned(d_out, out_stride, es)) return -1;
    const bool v16 = export_v16(d_out, out_stride, (size_t)(desc->planes == H264MI_RESID_UV ? desc->cw / 2 : desc->cw) * es);
    residual_args a;
    a.rec = (const uint8_t *)d_recs;
    a.coef = (const int16_t *)d_coef;
    a.coef_blocks = coef_blocks;
    a.w_mbs = w_mbs;
    a.x = desc->x; a.y = desc->y; a.cw = desc->cw; a.ch = desc->ch; a.planes = desc->planes;
    a.out_stride = out_stride;
    for (int c = 0; c < 3; c++) { a.scale[c] = desc->scale[c]; a.bias[c] = desc->bias[c]; }
    return export_launches(npics, rec_offsets, a.off, &a.out, d_out, out_stride, [&](int k0, int n) {
        for (int k = 0; k < RESID_MAX_PICS; k++) a.cbase[k] = k < n ? coef_bases[k0 + k] : 0;
        residual_launch(desc->dtype, v16, n, (hipStream_t)stream, a);
    });
}

// The kept records and coefficients of the slots (streams[k], slots[k]) as
// residual tensors in the caller's memory, ordered like
// h264mi_engine_export_mbinfo.  A slot whose coefficients are not held (nothing
// decoded into it since retention went on, forgotten, or more blocks than a
// batch holds) reads the spare 0xFF record batch: zeros.
extern "C" int h264mi_engine_export_residual(h264mi_engine *e, int n, const int *streams, const int *slots,
                                             const h264mi_residual_desc *desc, void *d_out, size_t out_stride,
                                             void *stream)
{
    if (!e || !e->d_keepc || !e->d_keep || n < 1 || !streams || !slots || !d_out || !residual_desc_ok(desc, e->w, e->h))
        return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->dtype), stream, [&] {
        const size_t nb = (size_t)e->nslots * e->nstreams;
        std::vector<size_t> off((size_t)n);
        std::vector<uint32_t> cbase((size_t)n);
        for (int k = 0; k < n; k++) {
            const size_t b = (size_t)streams[k] * e->nslots + slots[k];
            off[k] = sizeof(MbRec) * e->nmbs * (e->keepc_ok[b] ? b : nb);
            cbase[k] = (uint32_t)(b * keepc_cap(e));
        }
        return h264mi_residual_device(e->d_keep, off.data(), e->d_keepc, cbase.data(), nb * keepc_cap(e), n, e->w, e->h,
                                      desc, d_out, out_stride, e->st);
    });
}

// an export descriptor h264mi_accmv_device accepts on a w_mbs x h_mbs picture
static bool accmv_desc_ok(const h264mi_accmv_desc *d, int w_mbs, int h_mbs)
{
    return d && accmv_desc_fixed_ok(d) && accmv_window_ok(d, w_mbs, h_mbs);
}

// One step of the accumulated motion (accmv.hip k_accmv_step): the origin map
// of the picture whose records start at d_recs, from the maps d_ref_maps[s] of
// the slots it references (NULL: none) or, with key != 0, the identity.  Device
// pointers, asynchronous on `stream`.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_accmv_step_device(const void *d_recs, int w_mbs, int h_mbs, const void *const *d_ref_maps,
                                        int nslots, int key, void *d_map_out, void *stream)
{
    static_assert(H264MI_ACCMV_MAX_SLOTS == ACCMV_MAX_SLOTS && H264MI_ACCMV_MAX_CH == ACCMV_MAX_CH &&
                      H264MI_ACCMV_NCHANNELS == ACC_NCHANNELS && H264MI_ACCMV_ADX == ACC_ADX &&
                      H264MI_ACCMV_ADY == ACC_ADY && H264MI_ACCMV_JX == ACC_JX && H264MI_ACCMV_JY == ACC_JY &&
                      H264MI_ACCMV_ANCHORED == ACC_ANCHORED && ACCMV_MAX_PICS == EXPORT_MAX_PICS,
                  "include/h264mi.h and accmv.hip name the same channels and bounds");
    if (!d_recs || !d_map_out || !accmv_size_ok(w_mbs, h_mbs) || nslots < 0 || nslots > ACCMV_MAX_SLOTS ||
        (nslots && !d_ref_maps) || (((size_t)(uintptr_t)d_recs | (size_t)(uintptr_t)d_map_out) & 15))
        return -1;
    for (int s = 0; s < nslots; s++)
        if (d_ref_maps[s] == d_map_out || ((size_t)(uintptr_t)d_ref_maps[s] & 3)) return -1;
    accmv_step_args a;
    memset(&a, 0, sizeof(a));
    a.rec = (const uint8_t *)d_recs;
    a.w_mbs = w_mbs; a.W = 16 * w_mbs; a.H = 16 * h_mbs; a.nslots = nslots;
    a.out[0] = (uint32_t *)d_map_out;
    for (int s = 0; s < nslots; s++) a.ref[0][s] = (const uint32_t *)d_ref_maps[s];
    a.mode[0] = key ? ACCMV_KEY : ACCMV_STEP;
    accmv_step_launch(1, (hipStream_t)stream, a);
    HIPCHECK(hipGetLastError());
    return 0;
}

// a resized export's descriptor h264mi_accmv_resize_device accepts on a w_mbs x h_mbs picture
static bool accmv_resize_desc_ok(const h264mi_accmv_resize_desc *d, int w_mbs, int h_mbs)
{
    return d && accmv_resize_fixed_ok(d) && accmv_resize_window_ok(d, w_mbs, h_mbs);
}

// Both accumulated-motion exports (r != NULL: resized, desc = &r->f): one check
// and one fill of what their kernels share, accmv_args
static int accmv_device(const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                        const h264mi_accmv_desc *desc, const h264mi_accmv_resize_desc *r, void *d_out,
                        size_t out_stride, void *stream)
{
    if (!d_maps || !map_offsets || !d_out || npics < 1 || ((size_t)(uintptr_t)d_maps & 3) ||
        (r ? !accmv_resize_desc_ok(r, w_mbs, h_mbs) : !accmv_desc_ok(desc, w_mbs, h_mbs)))
        return -1;
    for (int k = 0; k < npics; k++)
        if (map_offsets[k] & 3) return -1;
    const size_t es = export_elem_size(desc->dtype);
    if (!export_aligned(d_out, out_stride, es)) return -1;
    const bool v16 = export_v16(d_out, out_stride, (size_t)desc->cw * es);
    fresize_args<fresize_accmv> ra;
    accmv_args &a = ra.f;
    a.maps = (const uint8_t *)d_maps;
    a.W = 16 * w_mbs;
    a.x = desc->x; a.y = desc->y; a.cw = desc->cw; a.ch = desc->ch; a.nch = desc->nch;
    a.out_stride = out_stride;
    for (int c = 0; c < ACCMV_MAX_CH; c++) {
        a.id[c] = c < desc->nch ? (uint8_t)desc->id[c] : 0;
        a.scale[c] = c < desc->nch ? desc->scale[c] : 0.0f;
        a.bias[c] = c < desc->nch ? desc->bias[c] : 0.0f;
    }
    ra.ow = r ? r->ow : 0; ra.oh = r ? r->oh : 0;
    return export_launches(npics, map_offsets, a.off, &a.out, d_out, out_stride, [&](int, int n) {
        if (r) fresize_launch(desc->dtype, n, (hipStream_t)stream, ra);
        else accmv_launch(desc->dtype, v16, n, (hipStream_t)stream, a);
    });
}

// Origin maps as planar channels (accmv.hip k_accmv): the window desc->(x, y,
// cw, ch) of the npics maps (16 * w_mbs words a row) that start map_offsets[k]
// bytes after d_maps, as contiguous (nch, ch, cw) elements of desc->dtype at
// d_out + k * out_stride; device pointers, asynchronous on `stream`;
// ACCMV_MAX_PICS pictures per launch.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_accmv_device(const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                                   const h264mi_accmv_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    return accmv_device(d_maps, map_offsets, npics, w_mbs, h_mbs, desc, NULL, d_out, out_stride, stream);
}

// The same fields resized (field_resize.hip): the window's integer field
// filtered to desc->oh x desc->ow samples per channel, picture k's (nch, oh, ow)
// elements at d_out + k * out_stride.  The window is at most 16384 a side and
// 32 times the output on each axis.  Stateless: the tap tables are made in the
// kernel.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_accmv_resize_device(const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                                          const h264mi_accmv_resize_desc *desc, void *d_out, size_t out_stride,
                                          void *stream)
{
    return accmv_device(d_maps, map_offsets, npics, w_mbs, h_mbs, desc ? &desc->f : NULL, desc, d_out, out_stride, stream);
}

// the maps of slots [first, first + n) of the engine's pool as (x, y, 0), on its stream
static int accmv_clear(h264mi_engine *e, size_t first, size_t n)
{
    accmv_step_args a;
    memset(&a, 0, sizeof(a));
    a.w_mbs = e->w; a.W = 16 * e->w; a.H = 16 * e->h;
    for (size_t k0 = 0; k0 < n; k0 += ACCMV_STEP_PICS) {
        const int m = n - k0 < ACCMV_STEP_PICS ? (int)(n - k0) : ACCMV_STEP_PICS;
        for (int k = 0; k < ACCMV_STEP_PICS; k++) {
            a.out[k] = e->d_acc + (first + k0 + (k < m ? k : 0)) * acc_words(e);
            a.mode[k] = ACCMV_CLEAR;
        }
        accmv_step_launch(m, e->st, a);
        HIPCHECK(hipGetLastError());
    }
    return 0;
}

// Origin-map retention: one map per (stream, slot), (x, y, 0) until a
// reconstruction into the slot steps into it (accmv_batch); every serial starts
// at 0, so switching on starts from nothing.  Off waits for the engine's stream
// (exports run on it) and frees.
extern "C" int h264mi_engine_keep_accmv(h264mi_engine *e, int on)
{
    if (!e) return -1;
    if ((on != 0) == (e->d_acc != NULL)) return 0;
    HIPCHECK(hipSetDevice(e->dev));
    if (on) {
        if (!accmv_size_ok(e->w, e->h) || e->nslots > ACCMV_MAX_SLOTS) return -1;
        const size_t nb = (size_t)e->nslots * e->nstreams;
        e->acc_key = (unsigned long long *)calloc((size_t)e->nstreams, sizeof(unsigned long long));
        e->acc_ser = (unsigned long long *)calloc(nb, sizeof(unsigned long long));
        if (!e->acc_key || !e->acc_ser || hipMalloc(&e->d_acc, nb * acc_words(e) * 4) != hipSuccess ||
            accmv_clear(e, 0, nb)) {
            (void)hipStreamSynchronize(e->st);
            (void)hipFree(e->d_acc);
            free(e->acc_key); free(e->acc_ser);
            e->d_acc = NULL; e->acc_key = e->acc_ser = NULL;
            return -1;
        }
        return 0;
    }
    if (h264mi_engine_keep_accres(e, 0)) return -1;     // the keys go with the maps they are read through
    HIPCHECK(hipStreamSynchronize(e->st));
    (void)hipFree(e->d_acc);
    free(e->acc_key); free(e->acc_ser);
    e->d_acc = NULL; e->acc_key = e->acc_ser = NULL;
    return 0;
}

// The kept maps of the slots (streams[k], slots[k]) as tensors in the caller's
// memory, ordered between the caller's stream and ours by export_ordered
static int engine_export_accmv(h264mi_engine *e, int n, const int *streams, const int *slots,
                               const h264mi_accmv_desc *desc, const h264mi_accmv_resize_desc *rdesc, void *d_out,
                               size_t out_stride, void *stream)
{
    if (!e || !e->d_acc || n < 1 || !streams || !slots || !d_out ||
        (rdesc ? !accmv_resize_desc_ok(rdesc, e->w, e->h) : !accmv_desc_ok(desc, e->w, e->h)))
        return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->dtype), stream, [&] {
        std::vector<size_t> off((size_t)n);
        for (int k = 0; k < n; k++) off[k] = acc_words(e) * 4 * ((size_t)streams[k] * e->nslots + slots[k]);
        return accmv_device(e->d_acc, off.data(), n, e->w, e->h, desc, rdesc, d_out, out_stride, e->st);
    });
}

extern "C" int h264mi_engine_export_accmv(h264mi_engine *e, int n, const int *streams, const int *slots,
                                          const h264mi_accmv_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    return engine_export_accmv(e, n, streams, slots, desc, NULL, d_out, out_stride, stream);
}

// the same, resized (h264mi_accmv_resize_device)
extern "C" int h264mi_engine_export_accmv_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                  const h264mi_accmv_resize_desc *desc, void *d_out, size_t out_stride,
                                                  void *stream)
{
    return engine_export_accmv(e, n, streams, slots, desc ? &desc->f : NULL, desc, d_out, out_stride, stream);
}

// an export descriptor h264mi_accres_device accepts on a w_mbs x h_mbs picture
static bool accres_desc_ok(const h264mi_accres_desc *d, int w_mbs, int h_mbs)
{
    return d && accres_desc_fixed_ok(d) && accres_window_ok(d, w_mbs, h_mbs);
}

// a resized export's descriptor h264mi_accres_resize_device accepts on a w_mbs x h_mbs picture
static bool accres_resize_desc_ok(const h264mi_accres_resize_desc *d, int w_mbs, int h_mbs)
{
    return d && accres_resize_fixed_ok(d) && accres_resize_window_ok(d, w_mbs, h_mbs);
}

// Both accumulated-residual exports (r != NULL: resized, desc = &r->f): one
// check and one fill of what their kernels share, accres_args
static int accres_device(const void *d_cur, const size_t *cur_offsets, const void *d_key, const size_t *key_offsets,
                         const void *d_maps, const size_t *map_offsets, int npics, int w_mbs, int h_mbs,
                         const h264mi_accres_desc *desc, const h264mi_accres_resize_desc *r, void *d_out,
                         size_t out_stride, void *stream)
{
    static_assert(H264MI_ACCRES_Y == ACCRES_Y && H264MI_ACCRES_UV == ACCRES_UV && H264MI_ACCRES_YUV == ACCRES_YUV &&
                      H264MI_ACCRES_RGB == ACCRES_RGB && ACCRES_MAX_PICS == EXPORT_MAX_PICS &&
                      H264MI_TENSOR_COLOUR_BT709_FULL == TENSOR_COLOUR_SETS - 1,
                  "include/h264mi.h and accres.hip name the same planes, bounds and colour sets");
    if (!d_cur || !cur_offsets || !key_offsets || !d_maps || !map_offsets || !d_out || npics < 1 ||
        (((size_t)(uintptr_t)d_cur | (size_t)(uintptr_t)d_key | (size_t)(uintptr_t)d_maps) & 3) ||
        (r ? !accres_resize_desc_ok(r, w_mbs, h_mbs) : !accres_desc_ok(desc, w_mbs, h_mbs)))
        return -1;
    for (int k = 0; k < npics; k++) {
        if ((map_offsets[k] | cur_offsets[k]) & 3) return -1;
        if (key_offsets[k] != (size_t)-1 && (!d_key || (key_offsets[k] & 3))) return -1;
    }
    const size_t es = export_elem_size(desc->dtype);
    if (!export_aligned(d_out, out_stride, es)) return -1;
    const int ow = desc->planes == H264MI_ACCRES_UV ? desc->cw / 2 : desc->cw;
    const bool v16 = export_v16(d_out, out_stride, (size_t)ow * es);
    fresize_args<fresize_accres> ra;
    accres_args &a = ra.f;
    a.cur = (const uint8_t *)d_cur; a.key = (const uint8_t *)d_key; a.maps = (const uint8_t *)d_maps;
    a.W = 16 * w_mbs; a.H = 16 * h_mbs; a.cpitch = H264MI_CPITCH(w_mbs);
    a.x = desc->x; a.y = desc->y; a.cw = desc->cw; a.ch = desc->ch;
    a.planes = desc->planes; a.zero = desc->unanchored == H264MI_ACCRES_ZERO;
    a.out_stride = out_stride;
    a.col = tensor_colour_sets[desc->colour];
    for (int c = 0; c < 3; c++) { a.scale[c] = desc->scale[c]; a.bias[c] = desc->bias[c]; }
    ra.ow = r ? r->ow : 0; ra.oh = r ? r->oh : 0;
    return export_launches(npics, map_offsets, a.map_off, &a.out, d_out, out_stride, [&](int k0, int n) {
        for (int k = 0; k < ACCRES_MAX_PICS; k++) {
            a.cur_off[k] = k < n ? cur_offsets[k0 + k] : 0;
            a.key_off[k] = k < n && key_offsets[k0 + k] != (size_t)-1 ? key_offsets[k0 + k] : ACCRES_NO_KEY;
        }
        if (r) fresize_launch(desc->dtype, n, (hipStream_t)stream, ra);
        else accres_launch(desc->dtype, v16, n, (hipStream_t)stream, a);
    });
}

// The accumulated residual (accres.hip k_accres): the window desc->(x, y, cw,
// ch) of npics pictures -- frame, key frame or none ((size_t)-1), origin map,
// each at its offset -- as contiguous (planes, ch, cw) elements of desc->dtype
// at d_out + k * out_stride; device pointers, asynchronous on `stream`;
// ACCRES_MAX_PICS pictures per launch.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_accres_device(const void *d_cur, const size_t *cur_offsets, const void *d_key,
                                    const size_t *key_offsets, const void *d_maps, const size_t *map_offsets, int npics,
                                    int w_mbs, int h_mbs, const h264mi_accres_desc *desc, void *d_out, size_t out_stride,
                                    void *stream)
{
    return accres_device(d_cur, cur_offsets, d_key, key_offsets, d_maps, map_offsets, npics, w_mbs, h_mbs, desc, NULL,
                         d_out, out_stride, stream);
}

// The same fields resized (field_resize.hip): the window's integer field (UV:
// its half-resolution grid) filtered to desc->oh x desc->ow samples per plane,
// picture k's (planes, oh, ow) elements at d_out + k * out_stride; the bounds of
// h264mi_accmv_resize_device on the grid.  -1 (nothing launched) on a bad argument.
extern "C" int h264mi_accres_resize_device(const void *d_cur, const size_t *cur_offsets, const void *d_key,
                                           const size_t *key_offsets, const void *d_maps, const size_t *map_offsets,
                                           int npics, int w_mbs, int h_mbs, const h264mi_accres_resize_desc *desc,
                                           void *d_out, size_t out_stride, void *stream)
{
    return accres_device(d_cur, cur_offsets, d_key, key_offsets, d_maps, map_offsets, npics, w_mbs, h_mbs,
                         desc ? &desc->f : NULL, desc, d_out, out_stride, stream);
}

static void accres_free(h264mi_engine *e)
{
    (void)hipFree(e->d_akey);
    free(e->akey_tag); free(e->akey_slot);
    e->d_akey = NULL; e->akey_tag = NULL; e->akey_slot = NULL;
    e->akey_n = 0;
}

// Key-picture retention: nkeys frames per stream, none tagged, so switching on
// starts from nothing (pictures decoded before have no key).  Off, and a change
// of nkeys, wait for the engine's stream (copies and exports run on it) and free.
extern "C" int h264mi_engine_keep_accres(h264mi_engine *e, int nkeys)
{
    if (!e || nkeys < 0 || nkeys > H264MI_ACCRES_MAX_KEYS) return -1;
    if (nkeys == e->akey_n) return 0;
    if (nkeys && !e->d_acc) return -1;          // a key is read through an origin map
    HIPCHECK(hipSetDevice(e->dev));
    if (e->akey_n) {
        HIPCHECK(hipStreamSynchronize(e->st));
        accres_free(e);
    }
    if (!nkeys) return 0;
    const size_t ne = (size_t)e->nstreams * nkeys;
    e->akey_tag = (unsigned long long *)calloc(ne, sizeof(unsigned long long));
    e->akey_slot = (int *)malloc(sizeof(int) * (size_t)e->nstreams);
    if (!e->akey_tag || !e->akey_slot || hipMalloc(&e->d_akey, ne * e->frame_bytes) != hipSuccess) {
        e->d_akey = NULL;
        accres_free(e);
        return -1;
    }
    for (int s = 0; s < e->nstreams; s++) e->akey_slot[s] = -1;
    e->akey_n = nkeys;
    return 0;
}

// the entry that holds the key of the slot's picture, or -1: the slot's map
// carries serial t, and entry t % akey_n holds that key iff it is tagged t
static long accres_entry(const h264mi_engine *e, int stream, int slot)
{
    const unsigned long long t = e->acc_ser[(size_t)stream * e->nslots + slot];
    const size_t entry = (size_t)stream * e->akey_n + (size_t)(t % (unsigned)e->akey_n);
    return t && e->akey_tag[entry] == t ? (long)entry : -1;
}

extern "C" int h264mi_engine_accres_held(h264mi_engine *e, int stream, int slot)
{
    if (!e || !e->d_akey || stream < 0 || stream >= e->nstreams || slot < 0 || slot >= e->nslots) return -1;
    return accres_entry(e, stream, slot) >= 0;
}

// The accumulated residual of the slots (streams[k], slots[k]) against the keys
// held for them, as tensors in the caller's memory, ordered between the
// caller's stream and ours by export_ordered
static int engine_export_accres(h264mi_engine *e, int n, const int *streams, const int *slots,
                                const h264mi_accres_desc *desc, const h264mi_accres_resize_desc *rdesc, void *d_out,
                                size_t out_stride, void *stream)
{
    if (!e || !e->d_akey || n < 1 || !streams || !slots || !d_out ||
        (rdesc ? !accres_resize_desc_ok(rdesc, e->w, e->h) : !accres_desc_ok(desc, e->w, e->h)))
        return -1;
    return export_ordered(e, n, streams, slots, d_out, out_stride, export_elem_size(desc->dtype), stream, [&] {
        std::vector<size_t> cur((size_t)n), key((size_t)n), map((size_t)n);
        for (int k = 0; k < n; k++) {
            const size_t b = (size_t)streams[k] * e->nslots + slots[k];
            const long entry = accres_entry(e, streams[k], slots[k]);
            cur[k] = e->frame_bytes * b;
            key[k] = entry < 0 ? (size_t)-1 : e->frame_bytes * (size_t)entry;
            map[k] = acc_words(e) * 4 * b;
        }
        return accres_device(e->d_frames, cur.data(), e->d_akey, key.data(), e->d_acc, map.data(), n, e->w, e->h, desc,
                             rdesc, d_out, out_stride, e->st);
    });
}

extern "C" int h264mi_engine_export_accres(h264mi_engine *e, int n, const int *streams, const int *slots,
                                           const h264mi_accres_desc *desc, void *d_out, size_t out_stride, void *stream)
{
    return engine_export_accres(e, n, streams, slots, desc, NULL, d_out, out_stride, stream);
}

// the same, resized (h264mi_accres_resize_device), under the same held-key rule
extern "C" int h264mi_engine_export_accres_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                   const h264mi_accres_resize_desc *desc, void *d_out,
                                                   size_t out_stride, void *stream)
{
    return engine_export_accres(e, n, streams, slots, desc ? &desc->f : NULL, desc, d_out, out_stride, stream);
}

extern "C" void *h264mi_engine_frame_ptr(h264mi_engine *e, int stream, int slot)
{
    if (!e) return NULL;
    return e->d_frames + e->frame_bytes * ((size_t)stream * e->nslots + slot);
}

extern "C" int h264mi_engine_abi(void) { return H264MI_ENGINE_ABI; }
extern "C" size_t h264mi_engine_frame_bytes(h264mi_engine *e) { return e ? e->pic_bytes : 0; }
extern "C" size_t h264mi_engine_slot_bytes(h264mi_engine *e) { return e ? e->frame_bytes : 0; }
extern "C" int h264mi_engine_chroma_pitch(h264mi_engine *e) { return e ? e->cpitch : 0; }

// neighbour-based concealment of a picture's missing MBs on the device
// (k_conceal, conceal.hip), behind the work already on the engine's stream:
// slot `slot` of stream `stream` holds the decoded MBs reconstructed with the
// loop filter off; order[0..n) are the MBs to conceal in h264bsdConceal's
// order, decoded[0..w*h) the MBs decoded (1) or missing (0).  The inputs are
// copied before returning.
static std::atomic<unsigned long long> g_conceal_launches{0};
// diagnostics: k_conceal launches in this process (tests: the device path ran)
extern "C" unsigned long long h264mi_conceal_launches(void) { return g_conceal_launches.load(); }
int engine_conceal_fits(const h264mi_engine *e) { return e && e->conceal_fits; }

extern "C" int h264mi_engine_conceal(h264mi_engine *e, int stream, int slot, const int *order, int n,
                                     const uint8_t *decoded)
{
    if (!e || stream < 0 || stream >= e->nstreams || slot < 0 || slot >= e->nslots || n < 0 || n > e->nmbs ||
        (n && (!order || !decoded)))
        return -1;
    if (!n) return 0;
    if (!e->conceal_fits) return -2;          // picture too large for k_conceal's LDS
    for (int i = 0; i < n; i++) if (order[i] < 0 || order[i] >= e->nmbs) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    const size_t bytes = (size_t)e->nmbs * (sizeof(int) + 1);
    if (!e->d_conceal) {
        HIPCHECK(hipMalloc(&e->d_conceal, bytes));
        HIPCHECK(hipHostMalloc(&e->h_conceal, bytes, hipHostMallocDefault));
        HIPCHECK(hipEventCreateWithFlags(&e->ev_conceal, hipEventDisableTiming));
    } else {
        HIPCHECK(hipEventSynchronize(e->ev_conceal));
    }
    memcpy(e->h_conceal, order, sizeof(int) * (size_t)n);
    memcpy(e->h_conceal + sizeof(int) * (size_t)e->nmbs, decoded, (size_t)e->nmbs);
    HIPCHECK(hipMemcpyAsync(e->d_conceal, e->h_conceal, bytes, hipMemcpyHostToDevice, e->st));
    HIPCHECK(hipEventRecord(e->ev_conceal, e->st));
    hipLaunchKernelGGL(k_conceal, dim3(1), dim3(64), (size_t)e->nmbs, e->st, (uint8_t *)h264mi_engine_frame_ptr(e, stream, slot),
                       e->w, e->h, e->cpitch, (const int *)e->d_conceal, n, (const uint8_t *)(e->d_conceal + sizeof(int) * (size_t)e->nmbs));
    HIPCHECK(hipGetLastError());
    g_conceal_launches++;
    // the slot's samples changed after its reconstruction: a key picture's copy is taken again
    if (e->d_akey && e->akey_slot[stream] == slot && accres_copy_key(e, stream, slot)) return -1;
    return 0;
}

extern "C" void *h264mi_device_alloc(size_t bytes)
{
    void *p = NULL;
    if (hipMalloc(&p, bytes) != hipSuccess) return NULL;
    return p;
}

extern "C" int h264mi_device_free(void *p) { return hipFree(p) == hipSuccess ? 0 : -1; }

extern "C" int h264mi_copy_h2d(void *dst, const void *src, size_t bytes)
{
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

// engine-scoped device memory: on the engine's GPU whatever the calling
// thread's current device is (one process per GPU: rank r's record batches
// must live on GPU r, next to its frame slots and launches)
extern "C" int h264mi_engine_device(const h264mi_engine *e) { return e ? e->dev : -1; }

extern "C" void *h264mi_engine_alloc(h264mi_engine *e, size_t bytes)
{
    if (!e || !bytes || hipSetDevice(e->dev) != hipSuccess) return NULL;
    void *p = NULL;
    if (hipMalloc(&p, bytes) != hipSuccess) return NULL;
    return p;
}

extern "C" int h264mi_engine_free(h264mi_engine *e, void *p)
{
    if (!e || hipSetDevice(e->dev) != hipSuccess) return -1;
    return hipFree(p) == hipSuccess ? 0 : -1;
}

extern "C" int h264mi_engine_copy_h2d(h264mi_engine *e, void *dst, const void *src, size_t bytes)
{
    if (!e || h264mi_pointer_device(dst) != e->dev) return -1;
    HIPCHECK(hipSetDevice(e->dev));
    HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->st));
    HIPCHECK(hipStreamSynchronize(e->st));
    return 0;
}

extern "C" int h264mi_pointer_device(const void *p)
{
    if (!p) return -1;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    if (at.type != hipMemoryTypeDevice) return -1;
    return at.device;
}

// -------- internal interface of the H264Backend adapter (engine_int.h) ----
hipStream_t engine_stream(h264mi_engine *e) { return e->st; }
unsigned *engine_err_words(h264mi_engine *e) { return e->d_err; }

void engine_shape(const h264mi_engine *e, int *w_mbs, int *h_mbs, int *nstreams, int *nslots, int *blocking)
{
    *w_mbs = e->w; *h_mbs = e->h; *nstreams = e->nstreams; *nslots = e->nslots;
    *blocking = e->ev_block != NULL;
}

int engine_poolable(const h264mi_engine *e) { return !e->tev && !e->d_prof; }

int engine_reuse(h264mi_engine *e)
{
    HIPCHECK(hipSetDevice(e->dev));
    engine_config(e);
    e->prepped_rec = e->prepped_pics = NULL;
    e->prepped_n = 0;
    e->err_accum = 0;
    e->err_bits = 0;          // the previous owner's device / checker flags
    e->steps = 1;
    e->last_kernel = NULL;
    if (h264mi_engine_keep_coefs(e, 0) || h264mi_engine_keep_records(e, 0) || h264mi_engine_keep_accmv(e, 0))
        return -1;                                                                          // the previous owner's retention
    // (keep_accmv(0) took the key pictures with it: h264mi_engine_keep_accres needs the maps, so it is never on without them)
    // the epoch keeps counting: the mailboxes hold tags of earlier launches only
    HIPCHECK(hipMemsetAsync(e->d_frames, 0, e->frame_bytes * e->nslots * e->nstreams, e->st));
    return 0;
}
