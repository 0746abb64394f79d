// H264Backend adapter of the HIP reconstruction engine (engine.hip) for the
// single-stream host decoder (decoder.c): per decoder instance a private
// engine, or a lane of the device's shared engine (h264mi_set_share); the
// pool of released engines and pinned output frames.  Plain host C++ over
// the HIP runtime API and the engine's internal interface (engine_int.h): no
// device code here, so that tests/null_device can build this file against a
// CPU stand-in of both and run its threading under TSan / ASan + UBSan.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <chrono>
#include <mutex>
#include <pthread.h>
#include <time.h>
#include "../hip/engine_int.h"
#include "decoder.h"

#define HIPCHECK(x)                                                                    \
    do {                                                                               \
        hipError_t err_ = (x);                                                         \
        if (err_ != hipSuccess) {                                                      \
            fprintf(stderr, "h264mi: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(err_), \
                    __FILE__, __LINE__);                                               \
            return -1;                                                                 \
        }                                                                              \
    } while (0)

// H264MI_BLOCKING_SYNC=1: an engine created now waits by sleeping
static int env_blocking()
{
    const char *v = getenv("H264MI_BLOCKING_SYNC");
    return v && atoi(v) ? 1 : 0;
}

// Released private engines, kept for the next decoder instance of the same
// shape: DecTestBench-style callers create one H264SwDec instance per stream
// (H264SwDecInit ... H264SwDecRelease), and a fresh engine costs ~20 device
// and pinned allocations, a stream, events and a frame clear.  A pooled
// engine is idle (its stream drained) and is handed out as a fresh one would
// be: frames cleared, no batch prepped, settings re-read.  H264MI_ENGINE_POOL=0
// turns it off; h264mi_pool_drain() frees what the pools hold (also run at
// process exit).
// at process exit the pools are drained by an atexit handler registered
// when something is first pooled -- after the HIP runtime initialised, so
// it runs before the runtime's own teardown (a library destructor would run
// too late in a process that loaded the runtime first, e.g. through torch)
extern "C" int h264mi_pool_drain(void);
static void pool_drain_at_exit() { (void)h264mi_pool_drain(); }
static void register_drain_once()
{
    static std::once_flag once;
    std::call_once(once, [] { atexit(pool_drain_at_exit); });
}

#define ENGINE_POOL_MAX 4
static std::mutex g_pool_mu;
static h264mi_engine *g_pool[ENGINE_POOL_MAX];
static std::atomic<unsigned long long> g_pool_reused, g_pool_created;

extern "C" void h264mi_engine_pool_stats(unsigned long long *reused, unsigned long long *created)
{
    if (reused) *reused = g_pool_reused.load();
    if (created) *created = g_pool_created.load();
}

static bool engine_pool_on()
{
    const char *v = getenv("H264MI_ENGINE_POOL");
    return !v || atoi(v) != 0;
}

static h264mi_engine *engine_get(int device, int w_mbs, int h_mbs, int nstreams, int nslots)
{
    h264mi_engine *e = NULL;
    const int blocking = env_blocking();
    if (engine_pool_on()) {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (int i = 0; i < ENGINE_POOL_MAX && !e; i++) {
            h264mi_engine *x = g_pool[i];
            int xw = 0, xh = 0, xs = 0, xn = 0, xb = 0;
            if (x) engine_shape(x, &xw, &xh, &xs, &xn, &xb);
            // the waits' kind (H264MI_BLOCKING_SYNC) is fixed when an engine is
            // created: it is part of the key
            if (x && h264mi_engine_device(x) == device && xw == w_mbs && xh == h_mbs && xs == nstreams &&
                xn == nslots && xb == blocking) {
                e = x;
                g_pool[i] = NULL;
            }
        }
    }
    if (!e) {
        g_pool_created++;
        return h264mi_engine_create(device, w_mbs, h_mbs, nstreams, nslots);
    }
    g_pool_reused++;
    if (engine_reuse(e)) { h264mi_engine_destroy(e); return NULL; }
    return e;
}

static void engine_put(h264mi_engine *e)
{
    if (!e) return;
    // engines with diagnostics state (timing events, profiling buffers) are not kept
    if (engine_pool_on() && engine_poolable(e) && hipSetDevice(h264mi_engine_device(e)) == hipSuccess &&
        hipStreamSynchronize(engine_stream(e)) == hipSuccess) {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (int i = 0; i < ENGINE_POOL_MAX; i++)
            if (!g_pool[i]) { g_pool[i] = e; register_drain_once(); return; }
    }
    h264mi_engine_destroy(e);
}

// -------- H264Backend adapter for the single-stream host decoder ----------

// Per-GPU shared engines (H264MI_SHARE=N, or h264mi_set_share): the decoder
// instances of a process that decode pictures of the same size on the same
// device share one engine of N lanes (one engine per picture size) (a lane = a stream index of the frame
// pool).  Each instance's H264SwDecDecode hands its picture's records to the
// batch being collected and returns once a launch has taken it: the batch
// launches when every attached instance has submitted, or SHARE_WAIT_US
// after its first picture -- one k_prep + k_wgpp launch for the pictures of
// up to N concurrent instances (threads) instead of one launch each.  The
// reference's multi-instance model is N independent instances
// (TestBenchMultipleInstance.c:134-305); each instance here still sees only
// its own pictures, in its own order.
#define SHARE_MAX 32
#define SHARE_SLOTS 17                    // MaxDpbFrames (16) + the current picture
#define SHARE_WAIT_US 1000                // default batch wait (H264MI_SHARE_WAIT_US)

struct HipBackendCtx;
struct SharedEng {
    std::mutex mu;
    // batch launched: a pthread condition on CLOCK_MONOTONIC, waited on with
    // pthread_cond_timedwait (std::condition_variable::wait_for waits through
    // pthread_cond_clockwait, which ThreadSanitizer builds of this toolchain
    // do not see release the mutex)
    pthread_cond_t cv;
    SharedEng()
    {
        pthread_condattr_t at;
        pthread_condattr_init(&at);
        pthread_condattr_setclock(&at, CLOCK_MONOTONIC);
        pthread_cond_init(&cv, &at);
        pthread_condattr_destroy(&at);
    }
    ~SharedEng() { pthread_cond_destroy(&cv); }
    int device, w, h, lanes;
    h264mi_engine *e;
    uint32_t used;                        // attached lanes
    int active;
    // the batch being collected
    int np;
    int stream[SHARE_MAX], slot[SHARE_MAX];
    const void *recs[SHARE_MAX];
    const int16_t *coefs[SHARE_MAX];
    uint32_t nc[SHARE_MAX];
    HipBackendCtx *who[SHARE_MAX];
    bool force[SHARE_MAX];                // test hook: start this picture with a device flag set
    bool heavy[SHARE_MAX];                // more than half the picture's MBs intra (launch_nmc)
    unsigned long long collecting, launched;   // batch ids: collecting > launched while np > 0
    // result of each launch, by batch id: a waiter whose batch was launched
    // by another thread reads its own batch's entry, however many batches
    // launched before it got the lock back
#define SHARE_RC_RING 64
    int rc_ring[SHARE_RC_RING];
};
static std::mutex g_share_mu;
#define SHARE_SIZES 4                     // shared engines per device, one per picture size
static SharedEng *g_share[16][SHARE_SIZES];
// totals per device; atomics, since share_launch runs under an engine's
// lock and the lock order is g_share_mu before SharedEng::mu
static std::atomic<unsigned long long> g_share_batches[16], g_share_pictures[16];
static int g_share_lanes = -1;            // -1: H264MI_SHARE from the environment
static int g_share_wait_us = SHARE_WAIT_US;

struct HipBackendCtx {
    int device;
    h264mi_engine *e;   // private engine, or the shared one's
    SharedEng *sh;      // shared engine (NULL: private)
    int lane;           // stream index in e
    hipEvent_t ev_last; // shared: after this instance's latest work on the engine stream
    uint8_t *d_rgba;    // shared: RGBA staging
    uint8_t **pref;     // per slot: host buffer a D2H copy of the slot's current picture was queued into
    // pinned, per frame slot: the device flags (ReconArgs::err: residual range,
    // expired bounded waits) of the picture reconstructed into the slot, copied
    // behind its launch -- a read reports the flags of the picture it reads,
    // whatever order pictures are output in and whatever else was read before
    unsigned *h_slot_err;
    // test hook (H264MI_DEBUG_FLAG_PICTURE=k): the k-th reconstruction of this
    // instance (1-based) starts with a forced device flag, to check that the
    // flag reaches exactly that picture's output whatever the output order
    unsigned ndecodes, force_flag_at;
    int nslots;
    unsigned enq, synced;   // work items queued on the engine's stream / of those, waited for by hb_sync
    bool keep[H264_KEEP_KINDS];     // asked for by the decoder, applied to every engine configured from then on
};

extern "C" int h264mi_set_share(int lanes)
{
    if (lanes < 0 || lanes > SHARE_MAX) return -1;
    std::lock_guard<std::mutex> g(g_share_mu);
    g_share_lanes = lanes;
    return 0;
}

static int share_lanes()
{
    std::lock_guard<std::mutex> g(g_share_mu);
    if (g_share_lanes < 0) {
        const char *v = getenv("H264MI_SHARE");
        const int n = v ? atoi(v) : 0;
        g_share_lanes = n > 1 && n <= SHARE_MAX ? n : 0;
        const char *w = getenv("H264MI_SHARE_WAIT_US");
        if (w && atoi(w) > 0) g_share_wait_us = atoi(w);
    }
    return g_share_lanes;
}

// caller holds sh->mu
static void share_launch(SharedEng *sh)
{
    if (sh->np == 0) return;
    h264mi_engine *e = sh->e;
    for (int i = 0; i < sh->np; i++)
        if (sh->force[i]) (void)hipMemsetAsync(engine_err_words(e) + i, 0x01, sizeof(unsigned), engine_stream(e));
    bool heavy = false;
    for (int i = 0; i < sh->np; i++) heavy |= sh->heavy[i];
    int rc = engine_decode_host(e, sh->np, sh->stream, sh->slot, sh->recs, sh->coefs, sh->nc, heavy ? 1 : 0);
    // each picture's device flags (ReconArgs::err, one word per batch
    // picture) into its instance's word for the slot it was reconstructed
    // into, then cleared for the next batch
    for (int i = 0; i < sh->np && rc == 0; i++)
        if (hipMemcpyAsync(sh->who[i]->h_slot_err + sh->slot[i], engine_err_words(e) + i, sizeof(unsigned),
                           hipMemcpyDeviceToHost, engine_stream(e)) != hipSuccess)
            rc = -1;
    if (hipMemsetAsync(engine_err_words(e), 0, sizeof(unsigned) * sh->np, engine_stream(e)) != hipSuccess) rc = -1;
    sh->rc_ring[sh->collecting % SHARE_RC_RING] = rc;
    for (int i = 0; i < sh->np; i++) (void)hipEventRecord(sh->who[i]->ev_last, engine_stream(e));
    g_share_batches[sh->device] += 1;
    g_share_pictures[sh->device] += (unsigned long long)sh->np;
    sh->np = 0;
    sh->launched = sh->collecting;
    sh->collecting++;
    pthread_cond_broadcast(&sh->cv);
}

static void share_detach(HipBackendCtx *c)
{
    SharedEng *sh = c->sh;
    if (!sh) return;
    std::lock_guard<std::mutex> g(g_share_mu);
    bool last;
    {
        std::unique_lock<std::mutex> l(sh->mu);
        sh->used &= ~(1u << c->lane);
        sh->active--;
        if (sh->np > 0 && sh->np >= sh->active) share_launch(sh);      // the others need not wait for us
        last = sh->active == 0;
        if (last) (void)hipStreamSynchronize(engine_stream(sh->e));
    }
    (void)hipEventDestroy(c->ev_last);
    (void)hipFree(c->d_rgba);
    c->ev_last = NULL; c->d_rgba = NULL;
    if (last) {
        for (int k = 0; k < SHARE_SIZES; k++)
            if (g_share[sh->device][k] == sh) g_share[sh->device][k] = NULL;
        h264mi_engine_destroy(sh->e);
        delete sh;
    }
    c->sh = NULL; c->e = NULL;
}

// attach to the device's shared engine for a w x h stream; 0 = attached
static int share_attach(HipBackendCtx *c, int w_mbs, int h_mbs, int nslots)
{
    const int lanes = share_lanes();
    if (lanes < 2 || nslots > SHARE_SLOTS || c->device < 0 || c->device >= 16) return -1;
    std::lock_guard<std::mutex> g(g_share_mu);
    SharedEng *sh = NULL;
    int free_k = -1;
    for (int k = 0; k < SHARE_SIZES; k++) {
        SharedEng *x = g_share[c->device][k];
        if (x && x->w == w_mbs && x->h == h_mbs) sh = x;
        else if (!x && free_k < 0) free_k = k;
    }
    if (!sh) {
        if (free_k < 0) return -1;                          // SHARE_SIZES sizes in use: a private engine
        h264mi_engine *e = h264mi_engine_create(c->device, w_mbs, h_mbs, lanes, SHARE_SLOTS);
        if (!e) return -1;
        sh = new SharedEng();
        sh->device = c->device; sh->w = w_mbs; sh->h = h_mbs; sh->lanes = lanes; sh->e = e;
        sh->used = 0; sh->active = 0; sh->np = 0; sh->collecting = 1; sh->launched = 0;
        g_share[c->device][free_k] = sh;
    }
    std::lock_guard<std::mutex> l(sh->mu);
    int lane = -1;
    for (int i = 0; i < sh->lanes; i++)
        if (!(sh->used & (1u << i))) { lane = i; break; }
    if (lane < 0) return -1;                                // all lanes taken: a private engine
    // a waiting instance sleeps (its core parses for another instance)
    if (hipEventCreateWithFlags(&c->ev_last, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess) return -1;
    (void)hipEventRecord(c->ev_last, engine_stream(sh->e));
    sh->used |= 1u << lane;
    sh->active++;
    c->sh = sh; c->lane = lane; c->e = sh->e;
    return 0;
}

// caller holds sh->mu: wait until batch `mine` was launched, at most the
// share wait; false on timeout
static bool wait_launched(SharedEng *sh, unsigned long long mine)
{
    struct timespec dl;
    clock_gettime(CLOCK_MONOTONIC, &dl);
    dl.tv_nsec += (long)g_share_wait_us * 1000;
    dl.tv_sec += dl.tv_nsec / 1000000000;
    dl.tv_nsec %= 1000000000;
    while (sh->launched < mine)
        if (pthread_cond_timedwait(&sh->cv, sh->mu.native_handle(), &dl) != 0 && sh->launched < mine) return false;
    return true;
}

// Weak like the crop and tensor entry points below: a backend built against
// the CPU stand-in of the engine leaves the kept fields' pairs NULL.
extern "C" int h264mi_engine_keep_records(h264mi_engine *e, int on) __attribute__((weak));
extern "C" int h264mi_engine_forget_records(h264mi_engine *e, int stream, int slot) __attribute__((weak));
extern "C" int h264mi_engine_keep_coefs(h264mi_engine *e, int on) __attribute__((weak));
extern "C" int h264mi_engine_keep_accmv(h264mi_engine *e, int on) __attribute__((weak));

// the decoder's switch for a kept field onto the instance's engine (hb_fields, below the exports)
static int hb_keep_apply(HipBackendCtx *c, int kind, bool on);

static int hb_configure(void *vctx, int w_mbs, int h_mbs, int nslots)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    if (c->sh) share_detach(c);
    else if (c->e) engine_put(c->e);
    c->e = NULL;
    free(c->pref);
    (void)hipHostFree(c->h_slot_err);
    c->h_slot_err = NULL;
    c->pref = (uint8_t **)calloc((size_t)nslots, sizeof(uint8_t *));
    c->nslots = c->pref ? nslots : 0;
    if (hipSetDevice(c->device) != hipSuccess ||
        hipHostMalloc(&c->h_slot_err, sizeof(unsigned) * (nslots > 0 ? nslots : 1), hipHostMallocDefault) != hipSuccess) {
        c->h_slot_err = NULL;
        return -1;
    }
    memset(c->h_slot_err, 0, sizeof(unsigned) * (nslots > 0 ? nslots : 1));
    if (share_attach(c, w_mbs, h_mbs, nslots) != 0) {
        c->lane = 0;
        c->e = engine_get(c->device, w_mbs, h_mbs, 1, nslots);
    }
    for (int k = 0; k < H264_KEEP_KINDS; k++)
        if (c->e && c->keep[k] && hb_keep_apply(c, k, true)) return -1;
    return c->e && c->pref ? 0 : -1;
}

static int hb_decode(void *vctx, const PicBuild *pb, int cur_slot)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    if (cur_slot >= 0 && cur_slot < c->nslots) c->pref[cur_slot] = NULL;
    c->enq++;
    const bool force = ++c->ndecodes == c->force_flag_at;
    if (!c->sh) {
        // (the slot is checked before anything is queued: a failed call
        // leaves no flag behind for the next picture)
        if (cur_slot < 0 || cur_slot >= c->nslots) return -1;
        h264mi_engine *e = c->e;
        hipStream_t st = engine_stream(e);
        if (force) HIPCHECK(hipMemsetAsync(engine_err_words(e), 0x01, sizeof(unsigned), st));
        int stream = 0;
        const void *recs[1] = {pb->rec};
        const int16_t *coefs[1] = {pb->coef};
        uint32_t nc[1] = {pb->ncoef};
        const int heavy = 2 * (int)pb->n_intra > pb->nmbs;
        // the decoder's own picture is in pinned memory (hb_host_alloc): uploaded
        // straight from it, the decoder waits (hb_records_wait) before reusing it
        if (pb->pinned ? engine_decode_direct(e, stream, cur_slot, pb->rec, pb->coef, pb->ncoef, heavy)
                       : engine_decode_host(e, 1, &stream, &cur_slot, recs, coefs, nc, heavy)) {
            (void)hipMemsetAsync(engine_err_words(e), 0, sizeof(unsigned), st);
            return -1;
        }
        // the picture's device flags into the slot's word, behind its launch
        HIPCHECK(hipMemcpyAsync(c->h_slot_err + cur_slot, engine_err_words(e), sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemsetAsync(engine_err_words(e), 0, sizeof(unsigned), st));
        return 0;
    }
    SharedEng *sh = c->sh;
    std::unique_lock<std::mutex> l(sh->mu);
    const int i = sh->np++;
    sh->stream[i] = c->lane; sh->slot[i] = cur_slot;
    sh->recs[i] = pb->rec; sh->coefs[i] = pb->coef; sh->nc[i] = pb->ncoef;
    sh->who[i] = c;
    sh->force[i] = force;
    sh->heavy[i] = 2 * (int)pb->n_intra > pb->nmbs;
    const unsigned long long mine = sh->collecting;
    if (sh->np >= sh->active) {
        share_launch(sh);
    } else if (!wait_launched(sh, mine)) {
        share_launch(sh);                 // the others are late: launch what is there
    }
    // (a waiter gets the lock back long before SHARE_RC_RING more batches
    // launch: each later batch takes a picture or a 1 ms wait of another instance)
    return sh->rc_ring[mine % SHARE_RC_RING];
}

static int hb_records_wait(void *vctx)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    // a shared engine's decode returns after its batch consumed the records
    if (c->sh || !c->e) return 0;
    return engine_records_wait(c->e);
}

static int hb_prefetch(void *vctx, int slot, uint8_t *dst)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    if (slot < 0 || slot >= c->nslots) return -1;
    h264mi_engine *e = c->e;
    HIPCHECK(hipSetDevice(h264mi_engine_device(e)));
    std::unique_lock<std::mutex> l;
    if (c->sh) l = std::unique_lock<std::mutex>(c->sh->mu);
    if (engine_copy_out(e, c->lane, slot, dst, engine_stream(e))) return -1;
    if (c->sh) HIPCHECK(hipEventRecord(c->ev_last, engine_stream(e)));
    c->pref[slot] = dst;
    c->enq++;
    return 0;
}

// the device flags of the picture in `slot` (ReconArgs::err: residual range,
// expired bounded waits), copied behind its launch into the slot's word,
// reach the caller as return 1; wait: sync first (the copy is stream-ordered)
static int slot_flagged(HipBackendCtx *c, int slot, bool wait = true)
{
    if (wait) {
        if (c->sh) HIPCHECK(hipEventSynchronize(c->ev_last));
        else if (engine_wait(c->e)) return -1;      // (flags: copied into h_slot_err behind each decode)
    }
    if (slot < 0 || slot >= c->nslots) return -1;
    const unsigned f = c->h_slot_err[slot];
    if (f) fprintf(stderr, "h264mi: device flagged the picture in slot %d (flags %#x)\n", slot, f);
    return f ? 1 : 0;
}

static int hb_sync(void *vctx)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    const unsigned n = c->enq;
    if (c->sh) {
        HIPCHECK(hipEventSynchronize(c->ev_last));
    } else if (engine_wait(c->e)) {
        return -1;
    }
    c->synced = n;
    return 0;
}

static int hb_read(void *vctx, int slot, uint8_t *dst)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    if (c->sh) {
        if (slot < 0 || slot >= c->nslots) return -1;
        if (c->pref[slot] != dst) {
            std::lock_guard<std::mutex> l(c->sh->mu);
            if (engine_copy_out(c->e, c->lane, slot, dst, engine_stream(c->e))) return -1;
            HIPCHECK(hipEventRecord(c->ev_last, engine_stream(c->e)));
        }
        return slot_flagged(c, slot);
    }
    // copied there already (hb_prefetch): only wait for it
    if (slot >= 0 && slot < c->nslots && c->pref[slot] == dst) return slot_flagged(c, slot, c->synced != c->enq);
    if (h264mi_engine_read(c->e, 0, slot, dst)) return -1;
    return slot_flagged(c, slot, false);
}

static int hb_read_rgba(void *vctx, int slot, uint8_t *dst)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    if (c->sh) {
        h264mi_engine *e = c->e;
        int w = 0, h = 0, ns = 0, nsl = 0, bl = 0;
        engine_shape(e, &w, &h, &ns, &nsl, &bl);
        const size_t bytes = (size_t)w * h * 256 * 4;
        if (slot < 0 || slot >= c->nslots) return -1;
        if (!c->d_rgba) HIPCHECK(hipMalloc(&c->d_rgba, bytes));
        {
            std::lock_guard<std::mutex> l(c->sh->mu);
            if (h264mi_yuv2rgba_device_pitch(h264mi_engine_frame_ptr(e, c->lane, slot), c->d_rgba, w * 16, h * 16,
                                             h264mi_engine_chroma_pitch(e), 1, 0, 0, engine_stream(e)))
                return -1;
            HIPCHECK(hipMemcpyAsync(dst, c->d_rgba, bytes, hipMemcpyDeviceToHost, engine_stream(e)));
            HIPCHECK(hipEventRecord(c->ev_last, engine_stream(e)));
        }
        return slot_flagged(c, slot);
    }
    if (h264mi_engine_read_rgba(c->e, 0, slot, dst)) return -1;
    return slot_flagged(c, slot, false);
}

// The crop entry points are weak here: the CPU stand-in of the engine
// (oracle/null_device.cpp) has none, and a backend built against it leaves read_crop NULL
// (H264SwDecNextPictureCropped then fails; there is no host crop).
extern "C" int h264mi_engine_read_crop(h264mi_engine *e, int stream, int slot, int x, int y, int cw, int ch, int rgba,
                                       uint8_t *dst) __attribute__((weak));
extern "C" int h264mi_crop_device_pitch(const void *d_in, void *d_out, int width, int height, int cpitch, int x, int y,
                                        int cw, int ch, int rgba, int npics, size_t in_stride, size_t out_stride,
                                        void *hip_stream) __attribute__((weak));

static int hb_read_crop(void *vctx, int slot, int x, int y, int cw, int ch, int rgba, uint8_t *dst)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    if (slot < 0 || slot >= c->nslots) return -1;
    if (c->sh) {
        h264mi_engine *e = c->e;
        int w = 0, h = 0, ns = 0, nsl = 0, bl = 0;
        engine_shape(e, &w, &h, &ns, &nsl, &bl);
        if (x < 0 || y < 0 || cw <= 0 || ch <= 0 || ((x | y | cw | ch) & 1) || cw > w * 16 - x || ch > h * 16 - y)
            return -1;
        const size_t bytes = rgba ? (size_t)cw * ch * 4 : (size_t)cw * ch * 3 / 2;
        // (the RGBA staging holds any crop of the picture in either form)
        if (!c->d_rgba) HIPCHECK(hipMalloc(&c->d_rgba, (size_t)w * h * 256 * 4));
        {
            std::lock_guard<std::mutex> l(c->sh->mu);
            if (h264mi_crop_device_pitch(h264mi_engine_frame_ptr(e, c->lane, slot), c->d_rgba, w * 16, h * 16,
                                         h264mi_engine_chroma_pitch(e), x, y, cw, ch, rgba, 1, 0, 0, engine_stream(e)))
                return -1;
            HIPCHECK(hipMemcpyAsync(dst, c->d_rgba, bytes, hipMemcpyDeviceToHost, engine_stream(e)));
            HIPCHECK(hipEventRecord(c->ev_last, engine_stream(e)));
        }
        return slot_flagged(c, slot);
    }
    if (h264mi_engine_read_crop(c->e, 0, slot, x, y, cw, ch, rgba, dst)) return -1;
    return slot_flagged(c, slot, false);
}

// Weak like the crop entry points: a backend built against the CPU stand-in of
// the engine leaves the exports NULL (H264SwDecNextPictureTensor then fails).
extern "C" int h264mi_engine_export_tensor(h264mi_engine *e, int n, const int *streams, const int *slots,
                                           const h264mi_tensor_desc *desc, void *d_out, size_t out_stride,
                                           void *hip_stream) __attribute__((weak));
extern "C" int h264mi_engine_export_tensor_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                   const h264mi_tensor_resize_desc *desc, void *d_out,
                                                   size_t out_stride, void *hip_stream) __attribute__((weak));
extern "C" int h264mi_engine_export_mbinfo(h264mi_engine *e, int n, const int *streams, const int *slots,
                                           const h264mi_mbinfo_desc *desc, void *d_out, size_t out_stride,
                                           void *hip_stream) __attribute__((weak));
extern "C" int h264mi_engine_export_residual(h264mi_engine *e, int n, const int *streams, const int *slots,
                                             const h264mi_residual_desc *desc, void *d_out, size_t out_stride,
                                             void *hip_stream) __attribute__((weak));
extern "C" int h264mi_engine_export_accmv(h264mi_engine *e, int n, const int *streams, const int *slots,
                                          const h264mi_accmv_desc *desc, void *d_out, size_t out_stride,
                                          void *hip_stream) __attribute__((weak));
extern "C" int h264mi_engine_export_accmv_resized(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                  const h264mi_accmv_resize_desc *desc, void *d_out, size_t out_stride,
                                                  void *hip_stream) __attribute__((weak));

// The exports of slot (desc: a checked descriptor of the engine call's
// kind) to d_dst.  Nothing waits here: the decoder synced before (the slot's
// flags are on the host), and the export orders itself on the engine's and the
// caller's stream.
template <class Desc>
static int hb_export(void *vctx, int slot,
                     int (*engine_export)(h264mi_engine *, int, const int *, const int *, const Desc *, void *, size_t, void *),
                     const void *desc, void *d_dst, void *hip_stream)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    if (!c->e || slot < 0 || slot >= c->nslots) return -1;
    const int lane = c->lane;
    std::unique_lock<std::mutex> l;
    if (c->sh) l = std::unique_lock<std::mutex>(c->sh->mu);
    if (engine_export(c->e, 1, &lane, &slot, (const Desc *)desc, d_dst, 0, hip_stream)) return -1;
    if (c->sh) HIPCHECK(hipEventRecord(c->ev_last, engine_stream(c->e)));
    c->enq++;
    return 0;
}

static int hb_export_tensor(void *vctx, int slot, const void *desc, void *d_dst, void *hip_stream)
{
    if (hb_export(vctx, slot, h264mi_engine_export_tensor, desc, d_dst, hip_stream)) return -1;
    return slot_flagged((HipBackendCtx *)vctx, slot, false);
}

static int hb_export_tensor_resized(void *vctx, int slot, const void *desc, void *d_dst, void *hip_stream)
{
    if (hb_export(vctx, slot, h264mi_engine_export_tensor_resized, desc, d_dst, hip_stream)) return -1;
    return slot_flagged((HipBackendCtx *)vctx, slot, false);
}

// A kept field's engine calls, by H264_KEEP_*: the retention switch and the export of slot
#define HB_EXPORT_AS(engine_export)                                                   \
    [](void *vctx, int slot, const void *desc, void *d_dst, void *hip_stream) {       \
        return hb_export(vctx, slot, engine_export, desc, d_dst, hip_stream);         \
    }
static const struct {
    int (*engine_keep)(h264mi_engine *, int);
    int (*export_field)(void *vctx, int slot, const void *desc, void *d_dst, void *hip_stream);
} hb_fields[H264_KEEP_KINDS] = {
    {h264mi_engine_keep_records, HB_EXPORT_AS(h264mi_engine_export_mbinfo)},
    {h264mi_engine_keep_coefs, HB_EXPORT_AS(h264mi_engine_export_residual)},
    {h264mi_engine_keep_accmv, HB_EXPORT_AS(h264mi_engine_export_accmv)},
};
#undef HB_EXPORT_AS
static_assert(H264_KEEP_RECORDS == 0 && H264_KEEP_COEFS == 1 && H264_KEEP_ACCMV == 2, "the order of hb_fields' rows");

// The decoder's switch `on` (c->keep[kind]) onto the instance's engine.  A
// shared engine's retention is only ever switched on: its other instances may
// be using it.
static int hb_keep_apply(HipBackendCtx *c, int kind, bool on)
{
    if (!c->sh) return hb_fields[kind].engine_keep(c->e, on);
    if (!on) return 0;
    std::lock_guard<std::mutex> l(c->sh->mu);
    return hb_fields[kind].engine_keep(c->e, 1);
}

static int hb_keep(void *vctx, int kind, int on)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    c->keep[kind] = on != 0;
    return c->e ? hb_keep_apply(c, kind, c->keep[kind]) : 0;
}

static int hb_export_field(void *vctx, int kind, int slot, const void *desc, void *d_dst, void *hip_stream)
{
    return hb_fields[kind].export_field(vctx, slot, desc, d_dst, hip_stream);
}

// the kept origin map of slot as the resized field (a member of its own, like export_tensor_resized)
static int hb_export_accmv_resized(void *vctx, int slot, const void *desc, void *d_dst, void *hip_stream)
{
    return hb_export(vctx, slot, h264mi_engine_export_accmv_resized, desc, d_dst, hip_stream);
}

// boxes of slot as resized tensors (a member of its own, with no retention):
// the list travels through hb_export as one descriptor, box r's elements
// packed behind box r - 1's
extern "C" int h264mi_engine_export_tensor_rois(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                const h264mi_tensor_resize_desc *desc, const h264mi_roi *rois,
                                                int nrois, void *d_out, size_t out_stride,
                                                void *hip_stream) __attribute__((weak));
struct RoisCall {
    const h264mi_tensor_resize_desc *desc;
    const h264mi_roi *rois;
    int nrois;
};

static int engine_export_rois(h264mi_engine *e, int n, const int *streams, const int *slots, const RoisCall *c,
                              void *d_out, size_t, void *hip_stream)
{
    const size_t planes = H264MI_TENSOR_LAYOUT(c->desc->t.mode) == H264MI_TENSOR_GRAY ? 1 : 3;
    return h264mi_engine_export_tensor_rois(e, n, streams, slots, c->desc, c->rois, c->nrois, d_out,
                                            planes * c->desc->oh * c->desc->ow * export_elem_size(c->desc->t.dtype),
                                            hip_stream);
}

static int hb_export_tensor_rois(void *vctx, int slot, const void *desc, const void *rois, int nrois, void *d_dst,
                                 void *hip_stream)
{
    const RoisCall c = {(const h264mi_tensor_resize_desc *)desc, (const h264mi_roi *)rois, nrois};
    return hb_export(vctx, slot, engine_export_rois, &c, d_dst, hip_stream);
}

// the two letterboxed exports (members of their own, like the ones above)
extern "C" int h264mi_engine_export_tensor_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                                               const h264mi_tensor_fit_desc *desc, void *d_out, size_t out_stride,
                                               void *hip_stream) __attribute__((weak));
extern "C" int h264mi_engine_export_tensor_rois_fit(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                    const h264mi_tensor_fit_desc *desc, const h264mi_roi *rois,
                                                    int nrois, void *d_out, size_t out_stride,
                                                    void *hip_stream) __attribute__((weak));
struct RoisFitCall {
    const h264mi_tensor_fit_desc *desc;
    const h264mi_roi *rois;
    int nrois;
};

static int hb_export_tensor_fit(void *vctx, int slot, const void *desc, void *d_dst, void *hip_stream)
{
    if (hb_export(vctx, slot, h264mi_engine_export_tensor_fit, desc, d_dst, hip_stream)) return -1;
    return slot_flagged((HipBackendCtx *)vctx, slot, false);
}

static int engine_export_rois_fit(h264mi_engine *e, int n, const int *streams, const int *slots, const RoisFitCall *c,
                                  void *d_out, size_t, void *hip_stream)
{
    const h264mi_tensor_resize_desc &r = c->desc->r;
    const size_t planes = H264MI_TENSOR_LAYOUT(r.t.mode) == H264MI_TENSOR_GRAY ? 1 : 3;
    return h264mi_engine_export_tensor_rois_fit(e, n, streams, slots, c->desc, c->rois, c->nrois, d_out,
                                                planes * r.oh * r.ow * export_elem_size(r.t.dtype), hip_stream);
}

static int hb_export_tensor_rois_fit(void *vctx, int slot, const void *desc, const void *rois, int nrois, void *d_dst,
                                     void *hip_stream)
{
    const RoisFitCall c = {(const h264mi_tensor_fit_desc *)desc, (const h264mi_roi *)rois, nrois};
    return hb_export(vctx, slot, engine_export_rois_fit, &c, d_dst, hip_stream);
}

// the pixel exports under a layout descriptor (a member of its own): the
// single-window form has export_tensor's returns, the list form packs box r's
// elements behind box r - 1's like export_tensor_rois
extern "C" int h264mi_engine_export_tensor_layout(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                  const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois,
                                                  int nrois, void *d_out, size_t out_stride,
                                                  void *hip_stream) __attribute__((weak));
struct LayoutCall {
    const h264mi_tensor_layout_desc *desc;
    const h264mi_roi *rois;
    int nrois;
};

static int engine_export_layout(h264mi_engine *e, int n, const int *streams, const int *slots, const LayoutCall *c,
                                void *d_out, size_t, void *hip_stream)
{
    const h264mi_tensor_resize_desc &r = c->desc->f.r;
    const size_t planes = H264MI_TENSOR_LAYOUT(r.t.mode) == H264MI_TENSOR_GRAY ? 1 : 3;
    return h264mi_engine_export_tensor_layout(e, n, streams, slots, c->desc, c->rois, c->nrois, d_out,
                                              c->rois ? planes * r.oh * r.ow * export_elem_size(r.t.dtype) : 0,
                                              hip_stream);
}

static int hb_export_tensor_layout(void *vctx, int slot, const void *desc, const void *rois, int nrois, void *d_dst,
                                   void *hip_stream)
{
    const LayoutCall c = {(const h264mi_tensor_layout_desc *)desc, (const h264mi_roi *)rois, nrois};
    if (hb_export(vctx, slot, engine_export_layout, &c, d_dst, hip_stream)) return -1;
    return rois ? 0 : slot_flagged((HipBackendCtx *)vctx, slot, false);
}

// the single-window form of the same into a strided destination (a member of its own)
extern "C" int h264mi_engine_export_tensor_dest(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                const h264mi_tensor_layout_desc *desc, const h264mi_roi *rois,
                                                int nrois, const h264mi_tensor_dest *dest, void *d_out,
                                                size_t out_stride, void *hip_stream) __attribute__((weak));
struct DestCall {
    const h264mi_tensor_layout_desc *desc;
    const h264mi_tensor_dest *dest;
};

static int engine_export_dest(h264mi_engine *e, int n, const int *streams, const int *slots, const DestCall *c,
                              void *d_out, size_t, void *hip_stream)
{
    return h264mi_engine_export_tensor_dest(e, n, streams, slots, c->desc, NULL, 0, c->dest, d_out, 0, hip_stream);
}

static int hb_export_tensor_dest(void *vctx, int slot, const void *desc, const void *dest, void *d_dst, void *hip_stream)
{
    const DestCall c = {(const h264mi_tensor_layout_desc *)desc, (const h264mi_tensor_dest *)dest};
    if (hb_export(vctx, slot, engine_export_dest, &c, d_dst, hip_stream)) return -1;
    return slot_flagged((HipBackendCtx *)vctx, slot, false);
}

// warps of slot as affine-warped tensors (a member of its own, with no
// retention): the list travels through hb_export as one descriptor, warp r's
// elements packed behind warp r - 1's
extern "C" int h264mi_engine_export_tensor_warps(h264mi_engine *e, int n, const int *streams, const int *slots,
                                                 const h264mi_tensor_warp_desc *desc, const h264mi_warp *warps,
                                                 int nwarps, void *d_out, size_t out_stride,
                                                 void *hip_stream) __attribute__((weak));
struct WarpsCall {
    const h264mi_tensor_warp_desc *desc;
    const h264mi_warp *warps;
    int nwarps;
};

static int engine_export_warps(h264mi_engine *e, int n, const int *streams, const int *slots, const WarpsCall *c,
                               void *d_out, size_t, void *hip_stream)
{
    const size_t planes = H264MI_TENSOR_LAYOUT(c->desc->t.mode) == H264MI_TENSOR_GRAY ? 1 : 3;
    return h264mi_engine_export_tensor_warps(e, n, streams, slots, c->desc, c->warps, c->nwarps, d_out,
                                             planes * c->desc->oh * c->desc->ow * export_elem_size(c->desc->t.dtype),
                                             hip_stream);
}

static int hb_export_tensor_warps(void *vctx, int slot, const void *desc, const void *warps, int nwarps, void *d_dst,
                                  void *hip_stream)
{
    const WarpsCall c = {(const h264mi_tensor_warp_desc *)desc, (const h264mi_warp *)warps, nwarps};
    return hb_export(vctx, slot, engine_export_warps, &c, d_dst, hip_stream);
}

// statistics of slot, of its window or of boxes over it (a member of its own,
// with no retention and no reference picture): the list travels through
// hb_export as one descriptor, item r's words packed behind item r - 1's
extern "C" int h264mi_engine_export_stats(h264mi_engine *e, int n, const int *streams, const int *slots,
                                          const int *ref_streams, const int *ref_slots, const h264mi_stats_desc *desc,
                                          const h264mi_roi *rois, int nrois, void *d_out, size_t out_stride,
                                          void *hip_stream) __attribute__((weak));
struct StatsCall {
    const h264mi_stats_desc *desc;
    const h264mi_roi *rois;
    int nrois;
};

static int engine_export_stats(h264mi_engine *e, int n, const int *streams, const int *slots, const StatsCall *c,
                               void *d_out, size_t, void *hip_stream)
{
    return h264mi_engine_export_stats(e, n, streams, slots, NULL, NULL, c->desc, c->rois, c->nrois, d_out,
                                      stats_item_words(c->desc) * 8, hip_stream);
}

static int hb_export_stats(void *vctx, int slot, const void *desc, const void *rois, int nrois, void *d_dst,
                           void *hip_stream)
{
    const StatsCall c = {(const h264mi_stats_desc *)desc, (const h264mi_roi *)rois, nrois};
    return hb_export(vctx, slot, engine_export_stats, &c, d_dst, hip_stream);
}

// Pinned host blocks (decoder output frames) kept after free for the next
// decoder instance: pinning tens of MB per instance is a large share of a
// short stream's host time.  Exact-size reuse, at most H264MI_HOST_POOL_MB
// (default 256: ten 1080p output frames and their headroom) kept per process;
// h264mi_pool_drain() returns them.
#define HOST_POOL_N 16
static size_t host_pool_cap()
{
    const char *v = getenv("H264MI_HOST_POOL_MB");
    const long mb = v ? atol(v) : 256;
    return mb > 0 ? (size_t)mb << 20 : 0;
}
static std::mutex g_hpool_mu;
static struct { void *p; size_t bytes; } g_hpool[HOST_POOL_N], g_hlive[4 * HOST_POOL_N];

static void *hb_host_alloc(void *vctx, size_t bytes)
{
    void *p = NULL;
    {
        std::lock_guard<std::mutex> g(g_hpool_mu);
        for (int i = 0; i < HOST_POOL_N && !p; i++)
            if (g_hpool[i].p && g_hpool[i].bytes == bytes) { p = g_hpool[i].p; g_hpool[i].p = NULL; }
    }
    if (!p && hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return NULL;
    std::lock_guard<std::mutex> g(g_hpool_mu);
    for (int i = 0; i < 4 * HOST_POOL_N; i++)
        if (!g_hlive[i].p) { g_hlive[i].p = p; g_hlive[i].bytes = bytes; break; }
    return p;
}

static void hb_host_free(void *vctx, void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_hpool_mu);
        size_t bytes = 0;
        for (int i = 0; i < 4 * HOST_POOL_N; i++)
            if (g_hlive[i].p == p) { bytes = g_hlive[i].bytes; g_hlive[i].p = NULL; break; }
        size_t kept = 0;
        for (int i = 0; i < HOST_POOL_N; i++) kept += g_hpool[i].p ? g_hpool[i].bytes : 0;
        if (bytes && engine_pool_on() && kept + bytes <= host_pool_cap())
            for (int i = 0; i < HOST_POOL_N; i++)
                if (!g_hpool[i].p) { g_hpool[i].p = p; g_hpool[i].bytes = bytes; register_drain_once(); return; }
    }
    (void)hipHostFree(p);
}

static int hb_conceal(void *vctx, int slot, const int *order, int n, const uint8_t *decoded)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    if (slot >= 0 && slot < c->nslots) c->pref[slot] = NULL;
    if (c->sh) {
        std::lock_guard<std::mutex> l(c->sh->mu);
        if (h264mi_engine_conceal(c->e, c->lane, slot, order, n, decoded)) return -1;
        HIPCHECK(hipEventRecord(c->ev_last, engine_stream(c->e)));
        return 0;
    }
    return h264mi_engine_conceal(c->e, c->lane, slot, order, n, decoded);
}

static int hb_conceal_ok(void *vctx)
{
    const HipBackendCtx *c = (const HipBackendCtx *)vctx;
    return c->e && engine_conceal_fits(c->e);
}

static int hb_copy(void *vctx, int dst, int src)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    if (dst >= 0 && dst < c->nslots) c->pref[dst] = NULL;
    bool kept = false;
    for (int k = 0; k < H264_KEEP_KINDS; k++) kept |= c->keep[k];
    if (c->sh) {
        std::lock_guard<std::mutex> l(c->sh->mu);
        HIPCHECK(hipMemcpyAsync(h264mi_engine_frame_ptr(c->e, c->lane, dst), h264mi_engine_frame_ptr(c->e, c->lane, src),
                                engine_slot_bytes(c->e), hipMemcpyDeviceToDevice, engine_stream(c->e)));
        // the copy is no reconstruction: dst's kept records say nothing about it
        if (kept && h264mi_engine_forget_records && h264mi_engine_forget_records(c->e, c->lane, dst)) return -1;
        HIPCHECK(hipEventRecord(c->ev_last, engine_stream(c->e)));
        return 0;
    }
    if (kept && h264mi_engine_forget_records && h264mi_engine_forget_records(c->e, 0, dst)) return -1;
    if (h264mi_engine_sync(c->e)) return -1;
    HIPCHECK(hipMemcpy(h264mi_engine_frame_ptr(c->e, 0, dst), h264mi_engine_frame_ptr(c->e, 0, src),
                       engine_slot_bytes(c->e), hipMemcpyDeviceToDevice));
    return 0;
}

static void hb_destroy(void *vctx)
{
    HipBackendCtx *c = (HipBackendCtx *)vctx;
    if (c->sh) share_detach(c);
    else if (c->e) engine_put(c->e);
    free(c->pref);
    (void)hipHostFree(c->h_slot_err);
    free(c);
}

// batches / pictures the device's shared engines launched since the process
// started; returns the instances attached now
extern "C" int h264mi_share_stats(int device, unsigned long long *batches, unsigned long long *pictures)
{
    if (device < 0 || device >= 16) return -1;
    std::lock_guard<std::mutex> g(g_share_mu);
    if (batches) *batches = g_share_batches[device].load();
    if (pictures) *pictures = g_share_pictures[device].load();
    int n = 0;
    for (int k = 0; k < SHARE_SIZES; k++) {
        SharedEng *sh = g_share[device][k];
        if (!sh) continue;
        std::lock_guard<std::mutex> l(sh->mu);
        n += sh->active;
    }
    return n;
}

extern "C" H264Backend h264mi_hip_backend_create(int device)
{
    H264Backend be;
    memset(&be, 0, sizeof(be));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        fprintf(stderr, "h264mi: no HIP device %d: the reconstruction path needs an MI355X\n", device);
        return be;                                  /* ctx == NULL: H264SwDecInit fails */
    }
    HipBackendCtx *c = (HipBackendCtx *)calloc(1, sizeof(HipBackendCtx));
    c->device = device;
    const char *ff = h264mi_test_hooks() ? getenv("H264MI_DEBUG_FLAG_PICTURE") : NULL;
    c->force_flag_at = ff && atoi(ff) > 0 ? (unsigned)atoi(ff) : 0;
    be.ctx = c;
    be.configure = hb_configure;
    be.decode = hb_decode;
    be.read = hb_read;
    be.read_rgba = hb_read_rgba;
    be.read_crop = h264mi_engine_read_crop && h264mi_crop_device_pitch ? hb_read_crop : NULL;
    be.export_tensor = h264mi_engine_export_tensor ? hb_export_tensor : NULL;
    be.export_tensor_resized = h264mi_engine_export_tensor_resized ? hb_export_tensor_resized : NULL;
    const bool mbinfo = h264mi_engine_keep_records && h264mi_engine_export_mbinfo;
    const bool have[H264_KEEP_KINDS] = {
        mbinfo,
        mbinfo && h264mi_engine_keep_coefs && h264mi_engine_export_residual,
        h264mi_engine_keep_accmv && h264mi_engine_export_accmv && h264mi_engine_forget_records,
    };
    for (int k = 0; k < H264_KEEP_KINDS; k++) {
        be.field[k].keep = have[k] ? hb_keep : NULL;
        be.field[k].export_field = have[k] ? hb_export_field : NULL;
    }
    be.export_accmv_resized = have[H264_KEEP_ACCMV] && h264mi_engine_export_accmv_resized ? hb_export_accmv_resized : NULL;
    be.export_tensor_rois = h264mi_engine_export_tensor_rois ? hb_export_tensor_rois : NULL;
    be.export_tensor_fit = h264mi_engine_export_tensor_fit ? hb_export_tensor_fit : NULL;
    be.export_tensor_rois_fit = h264mi_engine_export_tensor_rois_fit ? hb_export_tensor_rois_fit : NULL;
    be.export_tensor_layout = h264mi_engine_export_tensor_layout ? hb_export_tensor_layout : NULL;
    be.export_tensor_dest = h264mi_engine_export_tensor_dest ? hb_export_tensor_dest : NULL;
    be.export_tensor_warps = h264mi_engine_export_tensor_warps ? hb_export_tensor_warps : NULL;
    be.export_stats = h264mi_engine_export_stats ? hb_export_stats : NULL;
    be.host_alloc = hb_host_alloc;
    be.host_free = hb_host_free;
    be.records_wait = hb_records_wait;
    be.copy = hb_copy;
    // H264MI_HOST_CONCEAL=1: conceal on the host (a copy of the picture, conceal.c)
    be.conceal = getenv("H264MI_HOST_CONCEAL") && atoi(getenv("H264MI_HOST_CONCEAL")) ? NULL : hb_conceal;
    be.conceal_ok = hb_conceal_ok;
    be.sync = hb_sync;
    be.prefetch = hb_prefetch;
    be.destroy = hb_destroy;
    return be;
}

// Frees every engine and pinned frame the pools hold (engines and frames in
// use are not touched); returns how many engines were freed.  Also run at
// process exit (register_drain_once).
extern "C" int h264mi_pool_drain(void)
{
    h264mi_engine *eng[ENGINE_POOL_MAX];
    int n = 0;
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (int i = 0; i < ENGINE_POOL_MAX; i++)
            if (g_pool[i]) { eng[n++] = g_pool[i]; g_pool[i] = NULL; }
    }
    for (int i = 0; i < n; i++) h264mi_engine_destroy(eng[i]);
    void *blk[HOST_POOL_N];
    int m = 0;
    {
        std::lock_guard<std::mutex> g(g_hpool_mu);
        for (int i = 0; i < HOST_POOL_N; i++)
            if (g_hpool[i].p) { blk[m++] = g_hpool[i].p; g_hpool[i].p = NULL; g_hpool[i].bytes = 0; }
    }
    for (int i = 0; i < m; i++) (void)hipHostFree(blk[i]);
    return n;
}

// pooled engines and pinned bytes held right now (diagnostics, tests)
extern "C" void h264mi_pool_held(int *engines, size_t *pinned_bytes)
{
    int n = 0;
    size_t b = 0;
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (int i = 0; i < ENGINE_POOL_MAX; i++) n += g_pool[i] != NULL;
    }
    {
        std::lock_guard<std::mutex> g(g_hpool_mu);
        for (int i = 0; i < HOST_POOL_N; i++) b += g_hpool[i].p ? g_hpool[i].bytes : 0;
    }
    if (engines) *engines = n;
    if (pinned_bytes) *pinned_bytes = b;
}

