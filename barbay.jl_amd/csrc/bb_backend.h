// bb_backend.h -- the two backends of bb_engine.hip side by side: everything that differs between the product (hipcc, the
// HIP runtime) and the host emulation (g++ -DBB_EMU, one address space, kernels run block by block on the calling thread).
// Included only by bb_engine.hip, after the block-program headers and bb_fail.  Every primitive exists in both halves with
// the same signature, so that outside this file a conditional on BB_EMU only ever encloses whole functions or sections.
#pragma once

// ------------------------------------------------------------------------------------------------
// emulation
// ------------------------------------------------------------------------------------------------
#ifdef BB_EMU
#define BB_BACKEND_VERSION "barbay_hip 0.1 (host emulation, tests only)"
typedef int bbStream;
struct BackendState {};                // (the product's: graph, run timer, communicator)
struct DevGuard { explicit DevGuard(int) {} };

static int dmalloc(void** p, size_t n) { *p = calloc(1, n ? n : 1); return *p ? 0 : BB_ERR_DEVICE; }
static void dfree(void* p) { free(p); }
static int h2d(void* d, const void* h, size_t n, bbStream) { memcpy(d, h, n); return 0; }
static int d2h(void* h, const void* d, size_t n, bbStream) { memcpy(h, d, n); return 0; }
// `rows` rows of `width` bytes, pitches in bytes
static int h2d_2d(void* d, size_t dpitch, const void* h, size_t hpitch, size_t width, size_t rows, bbStream) {
    for (size_t r = 0; r < rows; ++r) memcpy((char*)d + r * dpitch, (const char*)h + r * hpitch, width);
    return 0;
}
static int d2d(void* d, const void* s, size_t n, bbStream) { memcpy(d, s, n); return 0; }
static int dzero(void* d, size_t n, bbStream) { memset(d, 0, n); return 0; }
static int dsync(bbStream) { return 0; }

// a kernel is a host function of one block: BB_KERNEL(threads, name, parameters...) { BB_CTX; block program with cx, BB_GRID }
#define BB_KERNEL(NT, name, ...) static void name(BBCtx& cx, int bb_grid, __VA_ARGS__)
#define BB_CTX (void)bb_grid
#define BB_GRID bb_grid
template <class F>
static void emu_launch(int nblocks, int nthr, size_t lds_doubles, F f) {
    std::vector<double> lds(lds_doubles + 64);
    for (int b = 0; b < nblocks; ++b) {
        BBCtx cx{nthr, b, lds.data()};
        f(cx);
    }
}
template <class... P, class... A>
static int launch(bbStream, void (*k)(BBCtx&, int, P...), int grid, int nthr, size_t lds_doubles, A&&... a) {
    emu_launch(grid, nthr, lds_doubles, [&](BBCtx& cx) { k(cx, grid, static_cast<P>(a)...); });
    return 0;
}
// the descriptor k_sample / k_update read through a pointer: the handle's own
template <class T> static const T* desc_ptr(const T*, const T* host) { return host; }
static std::string step_kernels_name(int) { return "emu:k_sample + k_update"; }

static int dev_check(int) { return 0; }
static int dev_cus(int, int fallback) { return fallback; }
static bool peer_enable(int, int) { return true; }
static int stream_open(bbStream*, BackendState&) { return 0; }
static void stream_quiesce(bbStream, BackendState&) {}
static void stream_close(bbStream) {}
static int hostmap_alloc(unsigned** host, unsigned** dev, size_t n) {
    *host = *dev = (unsigned*)calloc(n, sizeof(unsigned));
    return *host ? 0 : bb_fail(BB_ERR_DEVICE, "cannot allocate the host-mapped status words");
}
static void hostmap_free(unsigned* p) { free(p); }
static int finegrained_alloc(void** p, size_t n, bbStream) {
    *p = calloc(1, n);
    return *p ? 0 : bb_fail(BB_ERR_DEVICE, "out of memory");
}
static void finegrained_free(void* p) { free(p); }
// an "IPC handle" is the pointer itself
static int ipc_export(void* out, void* p) { memcpy(out, &p, sizeof(void*)); return 0; }
static int ipc_open(void** base, const void* src, void*) { memcpy(base, src, sizeof(void*)); return 0; }
static void ipc_close(void*) {}
static int timer_start(BackendState&, bbStream) { return 0; }
static int timer_stop(BackendState&, bbStream) { return 0; }
static int timer_wait(BackendState&, bbStream, double*) { return 0; }
// (no device to fit: every grid "fits", and k_persist is stepped also where its tile with the lambda table would not fit a CU's LDS)
static const char* resident_fit(const void*, int, size_t, int, int) { return nullptr; }
static const size_t PERSIST_LDS_CAP = ~(size_t)0;
static int probe_launch(bbStream, const DevState&, int, int, size_t, unsigned, unsigned** res) { *res = nullptr; return 0; }
static void probe_free(unsigned*) {}
// single address space: the "transport" is a pointer; check that every rank's inbox is distinct and writable
static int probe_collect(bbStream, unsigned*, const DevState& S, int world, int32_t* ok) {
    *ok = 0;
    for (int r = 0; r < world; ++r) {
        if (!S.xout_rdy[r]) return 0;
        for (int q = 0; q < r; ++q) if (S.xout_rdy[q] == S.xout_rdy[r]) return 0;
    }
    *ok = 1;
    return 0;
}
static bool comm_ready(const BackendState&) { return false; }
static int comm_make_id(void*) { return bb_fail(BB_ERR_COMM, "no RCCL in the emulation build"); }
static int comm_init(BackendState&, const void*, int, int, int) { return bb_fail(BB_ERR_COMM, "no RCCL in the emulation build"); }
static int comm_allreduce(BackendState&, bbStream, double*, size_t, int) {
    return bb_fail(BB_ERR_COMM, "in-library collectives are not available in the emulation build");
}

// ------------------------------------------------------------------------------------------------
// HIP
// ------------------------------------------------------------------------------------------------
#else
#include <dlfcn.h>
#define BB_BACKEND_VERSION "barbay_hip 0.1 (gfx950)"
typedef hipStream_t bbStream;
#define BB_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t _e = (call);                                                                   \
        if (_e != hipSuccess) return bb_fail(BB_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(_e)); \
    } while (0)
typedef void* bb_ncclComm_t;
struct BackendState {
    hipGraphExec_t graph = nullptr;    // the captured step loop (build_graph)
    int graph_steps = 0;
    bool graph_failed = false;         // capture / instantiation failed once (e.g. a collective that cannot be captured): stay eager
    unsigned launch_seq = 0;           // resident launches of this handle so far (RunArgs.launch_tag)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;      // the run timer
    bb_ncclComm_t comm = nullptr;
};
struct DevGuard {
    int prev = -1, dev;
    explicit DevGuard(int d) : dev(d) { if (d < 0) return; if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); }      // (d < 0: no guard)
    ~DevGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
    DevGuard(const DevGuard&) = delete;
    DevGuard& operator=(const DevGuard&) = delete;
};

static int dmalloc(void** p, size_t n) { BB_HIP(hipMalloc(p, n ? n : 1)); return 0; }
static void dfree(void* p) { (void)hipFree(p); }
static int h2d(void* d, const void* h, size_t n, bbStream s) {
    BB_HIP(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s));
    BB_HIP(hipStreamSynchronize(s));
    return 0;
}
static int d2h(void* h, const void* d, size_t n, bbStream s) {
    BB_HIP(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, s));
    BB_HIP(hipStreamSynchronize(s));
    return 0;
}
// `rows` rows of `width` bytes, pitches in bytes
static int h2d_2d(void* d, size_t dpitch, const void* h, size_t hpitch, size_t width, size_t rows, bbStream s) {
    BB_HIP(hipMemcpy2DAsync(d, dpitch, h, hpitch, width, rows, hipMemcpyHostToDevice, s));
    BB_HIP(hipStreamSynchronize(s));
    return 0;
}
static int d2d(void* d, const void* s_, size_t n, bbStream s) {
    BB_HIP(hipMemcpyAsync(d, s_, n, hipMemcpyDeviceToDevice, s));
    return 0;
}
static int dzero(void* d, size_t n, bbStream s) { BB_HIP(hipMemsetAsync(d, 0, n, s)); return 0; }
static int dsync(bbStream s) { BB_HIP(hipStreamSynchronize(s)); return 0; }

extern __shared__ __attribute__((aligned(16))) double bb_smem[];
#define BB_KERNEL(NT, name, ...) __global__ void __launch_bounds__(NT) name(__VA_ARGS__)
#define BB_CTX BBCtx cx{(int)blockDim.x, (int)blockIdx.x, bb_smem}
#define BB_GRID (int)gridDim.x
static int launch_check() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bb_fail(BB_ERR_DEVICE, "kernel launch: %s", hipGetErrorString(e));
    return 0;
}
// one small kernel on `s`: grid x nthr threads, `lds_doubles` of dynamic LDS (raised above the 64 KB default where needed)
template <class... P, class... A>
static int launch(bbStream s, void (*k)(P...), int grid, int nthr, size_t lds_doubles, A&&... a) {
    const size_t lds = lds_doubles * 8;
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return bb_fail(BB_ERR_DEVICE, "cannot raise dynamic LDS to %zu bytes", lds);
    hipLaunchKernelGGL(k, dim3(grid), dim3(nthr), lds, s, static_cast<P>(a)...);
    return launch_check();
}
// the descriptor k_sample / k_update read through a pointer: its device copy
template <class T> static const T* desc_ptr(const T* dev, const T*) { return dev; }
static std::string step_kernels_name(int kind) { return "k_sample<" + std::to_string(kind) + "> + k_update<" + std::to_string(kind) + ">"; }

static int dev_check(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return bb_fail(BB_ERR_DEVICE, "device %d: no such HIP device (%d visible)", device, ndev);
    return 0;
}
static int dev_cus(int device, int fallback) {
    hipDeviceProp_t pr;
    return hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount : fallback;
}
// device `di` may read and write `dj`'s memory (enabled now if it was not)
static bool peer_enable(int di, int dj) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, di, dj) != hipSuccess || !can) return false;
    DevGuard guard(di);
    hipError_t e = hipDeviceEnablePeerAccess(dj, 0);
    (void)hipGetLastError();
    return e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
}
// the handle's stream with the run timer's events; quiesce: drained, and all that hangs on it (graph, communicator, events) gone
static int stream_open(bbStream* s, BackendState& be) {
    hipError_t e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    if (e != hipSuccess) return bb_fail(BB_ERR_DEVICE, "hipStreamCreate: %s", hipGetErrorString(e));
    (void)hipEventCreate(&be.ev0);
    (void)hipEventCreate(&be.ev1);
    return 0;
}
static void comm_destroy(BackendState& be);
static void stream_quiesce(bbStream s, BackendState& be) {
    (void)hipStreamSynchronize(s);
    if (be.graph) (void)hipGraphExecDestroy(be.graph);
    comm_destroy(be);
    if (be.ev0) (void)hipEventDestroy(be.ev0);
    if (be.ev1) (void)hipEventDestroy(be.ev1);
}
static void stream_close(bbStream s) { if (s) (void)hipStreamDestroy(s); }
// words the kernels write and the host reads without a copy: host address, device address
static int hostmap_alloc(unsigned** host, unsigned** dev, size_t n) {
    void* hp = nullptr;
    void* dp = nullptr;
    if (hipHostMalloc(&hp, n * sizeof(unsigned), hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
        if (hp) (void)hipHostFree(hp);
        return bb_fail(BB_ERR_DEVICE, "cannot allocate the host-mapped status words");
    }
    memset(hp, 0, n * sizeof(unsigned));
    *host = (unsigned*)hp;
    *dev = (unsigned*)dp;
    return 0;
}
static void hostmap_free(unsigned* p) { if (p) (void)hipHostFree(p); }
// zeroed fine-grained device memory (remote stores and local polls must meet in memory, not in either side's L2)
static int finegrained_alloc(void** p, size_t n, bbStream s) {
    BB_HIP(hipExtMallocWithFlags(p, n, hipDeviceMallocFinegrained));
    BB_HIP(hipMemsetAsync(*p, 0, n, s));
    BB_HIP(hipStreamSynchronize(s));
    return 0;
}
static void finegrained_free(void* p) { if (p) (void)hipFree(p); }
static int ipc_export(void* out, void* p) {
    static_assert(sizeof(hipIpcMemHandle_t) <= BB_P2P_HANDLE_BYTES, "IPC handle does not fit");
    hipIpcMemHandle_t hnd;
    BB_HIP(hipIpcGetMemHandle(&hnd, p));
    memcpy(out, &hnd, sizeof hnd);
    return 0;
}
// (a peer's memory is mapped once: `mapped` is what an earlier import of this handle got)
static int ipc_open(void** base, const void* src, void* mapped) {
    if ((*base = mapped)) return 0;
    hipIpcMemHandle_t hnd;
    memcpy(&hnd, src, sizeof hnd);
    BB_HIP(hipIpcOpenMemHandle(base, hnd, hipIpcMemLazyEnablePeerAccess));
    return 0;
}
static void ipc_close(void* p) { (void)hipIpcCloseMemHandle(p); }
// the run timer: start and stop are stream events, wait drains the stream and reads the time between them
static int timer_start(BackendState& be, bbStream s) { BB_HIP(hipEventRecord(be.ev0, s)); return 0; }
static int timer_stop(BackendState& be, bbStream s) { BB_HIP(hipEventRecord(be.ev1, s)); return 0; }
static int timer_wait(BackendState& be, bbStream s, double* ms) {
    BB_HIP(hipStreamSynchronize(s));
    float t = 0;
    BB_HIP(hipEventElapsedTime(&t, be.ev0, be.ev1));
    *ms = t;
    return 0;
}
// Can all `grid` workgroups of resident kernel `k` (nthr threads, lds bytes of dynamic LDS) be on the device's `cus` compute units
// at once?  nullptr, or why not.
static const char* resident_fit(const void* k, int nthr, size_t lds, int grid, int cus) {
    int per_cu = 0;
    if (!k) return "no kernel instance";
    if (lds > 64 * 1024 && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return "cannot raise dynamic LDS";
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, nthr, lds) != hipSuccess) return "occupancy query failed";
    return (long long)per_cu * cus < grid ? "grid does not fit resident on the device" : nullptr;
}
static const size_t PERSIST_LDS_CAP = 160 * 1024;      // k_persist: the tile with its lambda table in one CU's LDS

// transport probe of the cross-GPU leg (the kernel: with the small kernels below), in two halves -- launch; collect, which frees the
// result buffer -- so that one host thread can run it on several devices at once
__global__ void k_p2p_probe_seq(DevState S, int rank, int world, size_t probe_words_off, unsigned seq, unsigned* result);
static int probe_launch(bbStream s, const DevState& S, int rank, int world, size_t probe_words_off, unsigned seq, unsigned** res) {
    BB_HIP(hipMalloc((void**)res, 64 * 4));
    BB_HIP(hipMemsetAsync(*res, 0, 64 * 4, s));
    return launch(s, k_p2p_probe_seq, 1, 64, 0, S, rank, world, probe_words_off, seq, *res);
}
static void probe_free(unsigned* res) { if (res) (void)hipFree(res); }
static int probe_collect(bbStream s, unsigned* res, const DevState&, int world, int32_t* ok) {
    unsigned host[64] = {0};
    *ok = 0;
    int rc = d2h(host, res, sizeof host, s);
    (void)hipFree(res);
    if (rc) return rc;
    int good = 1;
    for (int r = 0; r < world; ++r) good &= host[r] == 1u;
    *ok = good;
    return 0;
}

// ---- RCCL, bound at run time so that the library loads (and N = 1 runs) without it -------------
typedef struct { char internal[128]; } bb_ncclUniqueId;
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(bb_ncclUniqueId*) = nullptr;
    int (*CommInitRank)(bb_ncclComm_t*, int, bb_ncclUniqueId, int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, bb_ncclComm_t, hipStream_t) = nullptr;
    int (*CommDestroy)(bb_ncclComm_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
static int rccl_load() {
    if (g_rccl.lib) return 0;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (g_rccl.lib) break;
    }
    if (!g_rccl.lib) return bb_fail(BB_ERR_COMM, "cannot load librccl: %s", dlerror());
    g_rccl.GetUniqueId = (int (*)(bb_ncclUniqueId*))dlsym(g_rccl.lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(bb_ncclComm_t*, int, bb_ncclUniqueId, int))dlsym(g_rccl.lib, "ncclCommInitRank");
    g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, bb_ncclComm_t, hipStream_t))dlsym(g_rccl.lib, "ncclAllReduce");
    g_rccl.CommDestroy = (int (*)(bb_ncclComm_t))dlsym(g_rccl.lib, "ncclCommDestroy");
    g_rccl.GetErrorString = (const char* (*)(int))dlsym(g_rccl.lib, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy)
        return bb_fail(BB_ERR_COMM, "librccl lacks a required symbol");
    return 0;
}
static const char* rccl_error(int rc) { return g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error"; }
static bool comm_ready(const BackendState& be) { return be.comm != nullptr; }
static void comm_destroy(BackendState& be) { if (be.comm && g_rccl.CommDestroy) g_rccl.CommDestroy(be.comm); }
static int comm_make_id(void* id_out) {
    int rc = rccl_load();
    if (rc) return rc;
    bb_ncclUniqueId id;
    rc = g_rccl.GetUniqueId(&id);
    if (rc) return bb_fail(BB_ERR_COMM, "ncclGetUniqueId: %s", rccl_error(rc));
    memcpy(id_out, &id, sizeof id);
    return 0;
}
static int comm_init(BackendState& be, const void* id_in, int device, int world, int rank) {
    int rc = rccl_load();
    if (rc) return rc;
    BB_HIP(hipSetDevice(device));
    bb_ncclUniqueId id;
    memcpy(&id, id_in, sizeof id);
    rc = g_rccl.CommInitRank(&be.comm, world, id, rank);
    if (rc) { be.comm = nullptr; return bb_fail(BB_ERR_COMM, "ncclCommInitRank: %s", rccl_error(rc)); }
    return 0;
}
// in-place fp64 sum over the ranks
static int comm_allreduce(BackendState& be, bbStream s, double* buf, size_t n, int world) {
    if (!be.comm) return bb_fail(BB_ERR_COMM, "world_size = %d but bb_comm_init was not called (or use bb_step_moments/bb_step_apply)", world);
    int rc = g_rccl.AllReduce(buf, buf, n, /*ncclFloat64*/ 8, /*ncclSum*/ 0, be.comm, s);
    if (rc) return bb_fail(BB_ERR_COMM, "ncclAllReduce: %s", rccl_error(rc));
    return 0;
}
#endif

// ------------------------------------------------------------------------------------------------
// the small kernels: one declaration each, a __global__ wrapper of the block program in the product, a host function of one
// block in the emulation -- launch() takes either
// ------------------------------------------------------------------------------------------------
// (descriptors by pointer: scalar loads on demand; by value they cost dozens of SGPR spills per kernel)
template <int KIND>
BB_KERNEL(1024, k_sample, const DevModel* __restrict__ Mp, const DevState* __restrict__ Sp, RunArgs A, int NB) {
    const DevModel& M = *Mp;
    const DevState& S = *Sp;
    BB_CTX;
    bb_block_sample<KIND>(cx, M, S, A, NB);
}
template <int KIND>
BB_KERNEL(1024, k_update, const DevModel* __restrict__ Mp, const DevState* __restrict__ Sp, RunArgs A, int NB) {
    const DevModel& M = *Mp;
    const DevState& S = *Sp;
    BB_CTX;
    bb_block_update<KIND>(cx, M, S, A, NB);
}
BB_KERNEL(256, k_geno, DevModel M, DevState S, RunArgs A, int do_update, int do_sample, int upd_par) {
    BB_CTX;
    bb_block_geno(cx, M, S, A, BB_GRID, do_update, do_sample, upd_par);
}
BB_KERNEL(256, k_geno_sum, DevModel M, DevState S, long long m_lo, long long m_hi) {
    BB_CTX;
    bb_block_geno_sum(cx, M, S, BB_GRID, m_lo, m_hi);
}
BB_KERNEL(256, k_reduce, DevModel M, DevState S, int nblk, int ngeno_blocks) {
    BB_CTX;
    bb_block_reduce(cx, M, S, nblk, ngeno_blocks);
}
BB_KERNEL(256, k_theta_pack, DevModel M, DevState S, double* buf, int g_lo, int g_hi, int W, int unpack) {
    BB_CTX;
    bb_block_theta_pack(cx, M, S, buf, g_lo, g_hi, W, unpack, BB_GRID);
}
BB_KERNEL(256, k_init, DevModel M, DevState S, unsigned long long seed) {
    BB_CTX;
    bb_block_init(cx, M, S, seed, BB_GRID);
}
BB_KERNEL(1024, k_hier, HierArgs H) {
    BB_CTX;
    bb_block_hier(cx, H, BB_GRID);
}
BB_KERNEL(256, k_ppc_pop, PpcArgs P) {
    BB_CTX;
    bb_block_ppc_pop(cx, P, BB_GRID);
}
BB_KERNEL(1024, k_ppc, PpcArgs P) {
    BB_CTX;
    bb_block_ppc(cx, P, BB_GRID);
}
BB_KERNEL(256, k_freq_zpart, FreqArgs F) {
    BB_CTX;
    bb_block_freq_zpart(cx, F, BB_GRID);
}
BB_KERNEL(256, k_freq_zsum, FreqArgs F) {
    BB_CTX;
    bb_block_freq_zsum(cx, F, BB_GRID);
}
BB_KERNEL(1024, k_freq, FreqArgs F) {
    BB_CTX;
    bb_block_freq(cx, F, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_score, ScoreArgs A) {
    BB_CTX;
    bb_block_score(cx, A, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_loo, LooArgs A) {
    BB_CTX;
    bb_block_loo(cx, A, BB_GRID);
}
BB_KERNEL(256, k_rb_logz, RbArgs A) {
    BB_CTX;
    bb_block_rb_logz(cx, A, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_rb, RbArgs A) {
    BB_CTX;
    bb_block_rb(cx, A, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_rb_theta_part, ThetaArgs H) {
    BB_CTX;
    bb_block_theta_part(cx, H, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_rb_theta, ThetaArgs H) {
    BB_CTX;
    bb_block_theta(cx, H, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_rb_pop_part, PopArgs H) {
    BB_CTX;
    bb_block_pop_part(cx, H, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_rb_pop, PopArgs H) {
    BB_CTX;
    bb_block_pop(cx, H, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_rb_contrast, ContrastArgs C) {
    BB_CTX;
    bb_block_contrast(cx, C, BB_GRID);
}
BB_KERNEL(BB_DFE_PART_NT, k_dfe_part, DfeArgs D) {
    BB_CTX;
    bb_block_dfe_part(cx, D, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_dfe, DfeArgs D) {
    BB_CTX;
    bb_block_dfe(cx, D, BB_GRID);
}
BB_KERNEL(BB_RANK_VAL_NT, k_rank_val, RankArgs R) {
    BB_CTX;
    bb_block_rank_val(cx, R, BB_GRID);
}
BB_KERNEL(BB_RANK_SORT_NT, k_rank_sort, RankArgs R) {
    BB_CTX;
    bb_block_rank_sort(cx, R, BB_GRID);
}
BB_KERNEL(BB_RANK_SORT_NT, k_rank_merge, RankArgs R) {
    BB_CTX;
    bb_block_rank_merge(cx, R, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_rank_stats, RankArgs R) {
    BB_CTX;
    bb_block_rank_stats(cx, R, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_ls_bc, LsArgs L) {
    BB_CTX;
    bb_block_ls_bc(cx, L, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_ls_pop_part, LsArgs L) {
    BB_CTX;
    bb_block_ls_pop_part(cx, L, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_ls_pop, LsArgs L) {
    BB_CTX;
    bb_block_ls_pop(cx, L, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_lt_full, LtArgs L) {
    BB_CTX;
    bb_block_lt<BB_LT_FULL>(cx, L, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_lt_collapsed, LtArgs L) {
    BB_CTX;
    bb_block_lt<BB_LT_COLLAPSED>(cx, L, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_ll_part, LlArgs L) {
    BB_CTX;
    bb_block_ll_part(cx, L, BB_GRID);
}
BB_KERNEL(256, k_ll_sum, LlArgs L) {
    BB_CTX;
    bb_block_ll_sum(cx, L, BB_GRID);
}
BB_KERNEL(BB_SCORE_NT, k_ll, LlArgs L) {
    BB_CTX;
    bb_block_ll(cx, L, BB_GRID);
}
BB_KERNEL(BB_CHAIN_TNT, k_chain_transpose, ChainArgs C) {
    BB_CTX;
    bb_block_chain_transpose(cx, C, BB_GRID);
}
BB_KERNEL(BB_CHAIN_NT, k_chain_stats, ChainArgs C) {
    BB_CTX;
    bb_block_chain_stats(cx, C, BB_GRID);
}
BB_KERNEL(BB_TRACE_NT, k_trace_snapshot, TraceArgs T) {
    BB_CTX;
    bb_block_trace_snapshot(cx, T, BB_GRID);
}
BB_KERNEL(BB_TRACE_NT, k_trace_gather, TraceArgs T) {
    BB_CTX;
    bb_block_trace_gather(cx, T, BB_GRID);
}
BB_KERNEL(BB_TRACE_VNT, k_trace_verdict, TraceVerdictArgs V) {
    BB_CTX;
    bb_block_trace_verdict(cx, V);
}
// bb_logdensity_grad_batch (bb_logp.h): grid = tile + n_tiles * point
template <int KIND>
BB_KERNEL(1024, k_logp_moments, const DevModel* __restrict__ Mp, LogpArgs B, RunArgs A, int NB) {
    const DevModel& M = *Mp;
    BB_CTX;
    bb_block_logp_moments<KIND>(cx, M, B, A, NB);
}
template <int KIND>
BB_KERNEL(1024, k_logp_grad, const DevModel* __restrict__ Mp, LogpArgs B, RunArgs A, int NB) {
    const DevModel& M = *Mp;
    BB_CTX;
    bb_block_logp_grad<KIND>(cx, M, B, A, NB);
}
BB_KERNEL(256, k_logp_geno, const DevModel* __restrict__ Mp, LogpArgs B, int gsb) {
    const DevModel& M = *Mp;
    BB_CTX;
    bb_block_logp_geno(cx, M, B, gsb);
}
// bb_hmc_step (bb_hmc.h): grid = chunk + n_chunks * walker; k_hmc_reduce: grid = walkers
BB_KERNEL(BB_HMC_NT, k_hmc_momentum, HmcArgs H) {
    BB_CTX;
    bb_block_hmc_momentum(cx, H);
}
BB_KERNEL(BB_HMC_NT, k_hmc_kick_drift, HmcArgs H, int k) {
    BB_CTX;
    bb_block_hmc_kick_drift(cx, H, k);
}
BB_KERNEL(BB_HMC_NT, k_hmc_kick_energy, HmcArgs H, int k) {
    BB_CTX;
    bb_block_hmc_kick_energy(cx, H, k);
}
BB_KERNEL(64, k_hmc_reduce, HmcArgs H, int which, int k) {
    BB_CTX;
    bb_block_hmc_reduce(cx, H, which, k);
}
BB_KERNEL(BB_HMC_NT, k_hmc_keep, HmcArgs H) {
    BB_CTX;
    bb_block_hmc_keep(cx, H);
}
// bb_hmc_accum_* (bb_hmc_accum.h): k_hmc_accum on bb_hmc_step's grid; k_hmc_accum_stats: grid = pairs of latents / BB_HMC_NT
BB_KERNEL(BB_HMC_NT, k_hmc_accum, HmcArgs H, HmcAccArgs A) {
    BB_CTX;
    bb_block_hmc_accum(cx, H, A);
}
BB_KERNEL(BB_HMC_NT, k_hmc_accum_stats, HmcArgs H, HmcAccArgs A) {
    BB_CTX;
    bb_block_hmc_accum_stats(cx, H, A);
}
// bb_nuts_* (bb_nuts.h): on bb_hmc_step's grid; k_nuts_reduce: grid = walkers
BB_KERNEL(BB_HMC_NT, k_nuts_momentum, HmcArgs H, NutsArgs N) {
    BB_CTX;
    bb_block_nuts_momentum(cx, H, N);
}
BB_KERNEL(BB_HMC_NT, k_nuts_open, HmcArgs H, NutsArgs N) {
    BB_CTX;
    bb_block_nuts_open(cx, H, N);
}
BB_KERNEL(BB_HMC_NT, k_nuts_close, HmcArgs H, NutsArgs N) {
    BB_CTX;
    bb_block_nuts_close(cx, H, N);
}
BB_KERNEL(64, k_nuts_reduce, HmcArgs H, NutsArgs N) {
    BB_CTX;
    bb_block_nuts_reduce(cx, H, N);
}
BB_KERNEL(BB_HMC_NT, k_nuts_take, HmcArgs H, NutsArgs N) {
    BB_CTX;
    bb_block_nuts_take(cx, H, N);
}
#ifndef BB_EMU
// transport probe of the cross-GPU leg: this rank's token into every peer's inbox, then every peer's token here
__global__ void __launch_bounds__(64) k_p2p_probe_seq(DevState S, int rank, int world, size_t probe_words_off, unsigned seq, unsigned* result) {
    const int r = threadIdx.x;
    if (r < world) {
        unsigned* out = S.xout_rdy[r] + probe_words_off + 32 * rank;
        __hip_atomic_store(out, 0xB0000000u | (seq << 8) | (unsigned)rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const unsigned* in = S.xout_rdy[rank] + probe_words_off + 32 * r;
        const unsigned want = 0xB0000000u | (seq << 8) | (unsigned)r;
        unsigned seen = 0, spins = 0;
        while ((seen = __hip_atomic_load(in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) != want && ++spins < (1u << 22)) __builtin_amdgcn_s_sleep(2);
        result[r] = seen == want ? 1u : 0u;
    }
}
#endif
BB_KERNEL(256, k_normals, unsigned long long seed, unsigned step, unsigned stream, long long lo, long long hi, double* out) {
    BB_CTX;
    bb_block_normals(cx, seed, step, stream, lo, hi, out, BB_GRID);
}
BB_KERNEL(256, k_math, int fn, long long n, const double* x, const double* y, double* out0, double* out1) {
    BB_CTX;
    bb_block_math(cx, fn, n, x, y, out0, out1, BB_GRID);
}
