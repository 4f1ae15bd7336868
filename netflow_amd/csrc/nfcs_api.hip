// nfcs_api.hip — the C ABI (include/nfcs.h) over the gfx950 kernels: per-device context,
// argument checking, the device-resident entry point, the host-memory pipeline (pinned
// staging ring, H2D / kernel / D2H overlapped on two streams), synthetic batches, digests.
//
// Boundary being replaced: netflow::Packet::update_checksums() (packet.hpp:722-890), a void
// member that never throws and silently skips malformed packets. Here every entry point returns
// an int (0 or a negative NFCS_E*), never throws, and reports per-packet outcomes as status bytes.
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

#include "nfcs_internal.h"
#include "nfcs_store_policy.h"

// Pinned host memory for the staging ring, on the GPU's NUMA node when that is known: mmap'd,
// bound to the node (mbind, MPOL_PREFERRED), faulted in there, then registered with HIP; else
// hipHostMalloc.
struct HostBlock {
    void* p = nullptr;
    size_t bytes = 0;
    bool mapped = false;  // mmap + hipHostRegister (free with hipHostUnregister + munmap)
};

// A fixed set of host threads for the host path's staging copies, gathers and checksum write-back,
// pinned to the GPU's NUMA node (round 5: started once with the staging ring, instead of threads
// spawned per copy). run(k, fn) runs fn(0) .. fn(k-1) over the workers and the calling thread and
// returns when all are done; with no worker (none could be started) the caller runs them all.
// Never throws: a thread that cannot be started is simply not there.
class Workers {
public:
    ~Workers() { stop(); }
    void start(int n, const cpu_set_t* cpus) noexcept {
        for (int i = 0; i < n; ++i) {
            try {
                th_.emplace_back([this, cpus] { loop(cpus); });
            } catch (...) {
                break;
            }
        }
    }
    void stop() noexcept {
        {
            std::lock_guard<std::mutex> l(mu_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
        th_.clear();
        quit_ = false;
    }
    int size() const { return (int)th_.size(); }
    // fn is called by reference, never copied (no allocation: nothing here can throw)
    template <class F>
    void run(int k, const F& fn) noexcept {
        if (k <= 1 || th_.empty()) {
            for (int i = 0; i < k; ++i) fn(i);
            return;
        }
        run_erased(k, [](const void* f, int i) { (*(const F*)f)(i); }, &fn);
    }

private:
    void run_erased(int k, void (*call)(const void*, int), const void* fn) noexcept {
        std::unique_lock<std::mutex> l(mu_);
        call_ = call;
        job_ = fn;
        parts_ = k;
        next_ = 0;
        pending_ = k;
        ++gen_;
        cv_.notify_all();
        take(l);  // the caller works too
        done_.wait(l, [&] { return pending_ == 0; });
        job_ = nullptr;
    }
    void take(std::unique_lock<std::mutex>& l) {
        while (next_ < parts_) {
            const int i = next_++;
            void (*const call)(const void*, int) = call_;
            const void* const f = job_;
            l.unlock();
            call(f, i);
            l.lock();
            if (--pending_ == 0) done_.notify_all();
        }
    }
    void loop(const cpu_set_t* cpus) {
        if (cpus) (void)pthread_setaffinity_np(pthread_self(), sizeof(cpu_set_t), cpus);
        std::unique_lock<std::mutex> l(mu_);
        uint64_t seen = 0;
        for (;;) {
            cv_.wait(l, [&] { return quit_ || (gen_ != seen && next_ < parts_); });
            if (quit_) return;
            take(l);
            seen = gen_;
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    void (*call_)(const void*, int) = nullptr;
    const void* job_ = nullptr;
    int parts_ = 0, next_ = 0, pending_ = 0;
    uint64_t gen_ = 0;
    bool quit_ = false;
};

struct nfcs_ctx {
    nfcs::DevInfo di;
    int numa_node = -1;     // the GPU's NUMA node (sysfs), -1 if unknown
    bool numa_local = false;  // staging memory bound to it
    bool have_cpus = false;   // copy threads pinned to its CPUs
    cpu_set_t node_cpus;
    HostBlock hb[2];
    hipStream_t stream = nullptr;
    // host pipeline (nfcs_update_host)
    static constexpr int kSlots = 2;
    static constexpr size_t kStageBytes = size_t(64) << 20;  // arena bytes per staging slot
    bool host_ready = false;  // every staging slot allocated (ensure_host_pipeline)
    hipStream_t hs[kSlots] = {nullptr, nullptr};
    hipEvent_t done[kSlots] = {nullptr, nullptr};    // a slot's chunk finished (records / frames back)
    hipEvent_t staged[kSlots] = {nullptr, nullptr};  // a slot's host arena and descriptors copied in
    size_t stage_bytes = 0;   // arena bytes per slot
    uint32_t stage_pkts = 0;  // descriptors per slot
    int copy_threads = 8;     // host threads for pageable <-> pinned staging copies
    Workers workers;          // copy_threads - 1 of them (the calling thread is the last)
    uint8_t* d_arena[kSlots] = {nullptr, nullptr};
    nfcs_desc* d_desc[kSlots] = {nullptr, nullptr};
    uint8_t* d_status[kSlots] = {nullptr, nullptr};
    nfcs_patch* d_patch[kSlots] = {nullptr, nullptr};
    // direct chunks' completion flags (nfcs::DoneReq): per slot a host-mapped word on its own 64-byte
    // line (done_host[8 s]), a device counter of finished workgroups, and the count the slot's next
    // launch starts from; wait_for[s] != 0: the chunk in slot s signals through its flag
    uint64_t* done_host = nullptr;
    uint64_t* done_dev = nullptr;
    uint64_t* done_ctr = nullptr;
    uint64_t done_base[kSlots] = {0, 0};
    int slot_wait[kSlots] = {0, 0};  // 0: the slot's chunk is waited for on its event; 1: on its flag; 2: flag seen
    uint8_t* z_block[kSlots] = {nullptr, nullptr};  // the pinned block of each slot as the GPU addresses it
                                                    // (direct chunks; null: not mapped, DMA only)
    uint8_t* h_arena[kSlots] = {nullptr, nullptr};  // pinned
    nfcs_desc* h_desc[kSlots] = {nullptr, nullptr};
    uint8_t* h_status[kSlots] = {nullptr, nullptr};
    nfcs_patch* h_patch[kSlots] = {nullptr, nullptr};
    uint64_t* d_digest = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // patch records of the waves that defer their stores (kUpdateAuto without a caller d_patch),
    // grown on demand; its last user ran on ws_stream (ws_own: the context's own stream). ws_ev
    // marks that user's write pass: recorded by the call itself on a caller's stream, and only when
    // another stream comes along on the context's own one (acquire_ws)
    nfcs_patch* ws = nullptr;
    size_t ws_cap = 0;  // records
    hipEvent_t ws_ev = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_used = false;
    bool ws_own = false;
    // nfcs_egress_enqueue_device's scratch (tile histograms, totals, rooms), grown on demand; its last
    // user ran on eq_stream, and eq_ev orders a call on another stream behind it, as ws_ev does for ws
    uint32_t* eq_ws = nullptr;
    uint64_t eq_cap = 0;  // words
    hipEvent_t eq_ev = nullptr;
    hipStream_t eq_stream = nullptr;
    bool eq_used = false;
    bool eq_own = false;
    // the stage counters' stripes (nfcs_internal.h kCtSlots; all zero between launches), allocated by the first
    // call that counts; ct_ev orders a call on another stream behind the last user's fold, as eq_ev does for eq_ws
    uint64_t* ct_ws = nullptr;
    hipEvent_t ct_ev = nullptr;
    hipStream_t ct_stream = nullptr;
    bool ct_used = false;
    bool ct_own = false;
    uint32_t slot_bytes = 0;  // launch-shape hint (nfcs_ctx_set_slot_bytes); 0 = arena_bytes / n
    // the footprint observations (launch_shape): kObsSlots host-mapped 64-bit slots the kernels
    // write ({generation, mean}), one per recently seen burst (descriptor array, n, arena bytes),
    // least recently used replaced; so calls rotating over a few bursts (a ring's descriptor arrays,
    // the bench's batches) each adapt, and a late sample of a replaced burst is ignored
    static constexpr int kObsSlots = 8;
    uint64_t* obs_host = nullptr;
    uint64_t* obs_dev = nullptr;
    struct ObsBurst { const void* desc; uint32_t n; uint64_t bytes; uint32_t gen; uint64_t used; };
    ObsBurst obs_burst[kObsSlots] = {};
    uint32_t obs_gen = 0;   // the last generation handed out (0: never; slots start empty)
    uint64_t obs_clock = 0;
    // Store demand (nfcs_internal.h DemandReq, nfcs_store_policy.h): two buffers of counter words in
    // device memory, alternating by the call's generation; the host-mapped word the next call forwards a
    // call's count to; how many packets each of the last calls sampled (the host knows it from n alone);
    // and the policy over the observations read so far. dem_last_form: the form the newest update call
    // ran in (NFCS_STORE_DEFERRED / NFCS_STORE_SPARSE; 0: none yet, or a call the forms do not apply to).
    static constexpr int kDemRing = 64;  // calls the host may be ahead of the device and still place an observation
    uint32_t* dem_dev = nullptr;
    uint64_t* dem_host = nullptr;
    uint64_t* dem_host_dev = nullptr;
    uint32_t dem_gen = 0;
    struct DemCall { uint32_t gen, sampled; };
    DemCall dem_calls[kDemRing] = {};
    nfcs::StorePolicy dem_policy;
    int store_policy = NFCS_STORE_AUTO;
    int dem_last_form = 0;
    hipStream_t dem_stream = nullptr;
    bool dem_any = false;  // dem_stream is the stream of the previous update call
};

namespace {

thread_local int g_last_hip = 0;

// The deferred-store workspace for a launch of n packets on `st`. A launch on another stream
// than the previous user first waits (on the device) for that user's write pass, so calls on one
// context from several streams never overwrite each other's records; growing it waits on the host.
// A previous user on the context's own stream gets its event here, when it is needed: that stream
// lives as long as the context, and an event recorded now follows all its work. So back-to-back
// calls on one stream queue nothing between their kernels (an event per call cost C1 ~6 µs of idle
// GPU between calls, 1.5-2%; round 3, profiles/r03_s3_ab_ws_event.jsonl).
hipError_t wait_ws_user(nfcs_ctx* c, hipStream_t st) {
    if (c->ws_own) {
        hipError_t e = hipEventRecord(c->ws_ev, c->stream);
        if (e != hipSuccess) return e;
    }
    return st ? hipStreamWaitEvent(st, c->ws_ev, 0) : hipEventSynchronize(c->ws_ev);
}

hipError_t acquire_ws(nfcs_ctx* c, size_t n, hipStream_t st) {
    if (n > c->ws_cap) {
        if (c->ws_used) {
            hipError_t e = wait_ws_user(c, nullptr);  // on the host: the buffer is freed next
            if (e != hipSuccess) return e;
        }
        if (c->ws) (void)hipFree(c->ws);
        c->ws = nullptr;
        c->ws_cap = 0;
        c->ws_used = false;
        const size_t cap = n < (1u << 20) ? (1u << 20) : n;
        hipError_t e = hipMalloc(&c->ws, cap * sizeof(nfcs_patch));
        if (e != hipSuccess) return e;
        c->ws_cap = cap;
    } else if (c->ws_used && c->ws_stream != st) {
        hipError_t e = wait_ws_user(c, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t release_ws(nfcs_ctx* c, hipStream_t st) {
    c->ws_stream = st;
    c->ws_used = true;
    c->ws_own = st == c->stream;
    // a caller's stream may be gone by the time another stream comes: its event is recorded now
    return c->ws_own ? hipSuccess : hipEventRecord(c->ws_ev, st);
}

// The same for the enqueue's scratch (eq_ws): `words` words for a launch on `st`. A failed allocation
// leaves the context without scratch and otherwise as it was.
hipError_t wait_eq_user(nfcs_ctx* c, hipStream_t st) {
    if (c->eq_own) {
        hipError_t e = hipEventRecord(c->eq_ev, c->stream);
        if (e != hipSuccess) return e;
    }
    return st ? hipStreamWaitEvent(st, c->eq_ev, 0) : hipEventSynchronize(c->eq_ev);
}
hipError_t acquire_eq(nfcs_ctx* c, uint64_t words, hipStream_t st) {
    if (words > c->eq_cap) {
        if (c->eq_used) {
            hipError_t e = wait_eq_user(c, nullptr);  // on the host: the buffer is freed next
            if (e != hipSuccess) return e;
        }
        if (c->eq_ws) (void)hipFree(c->eq_ws);
        c->eq_ws = nullptr;
        c->eq_cap = 0;
        c->eq_used = false;
        const uint64_t cap = words < (1u << 18) ? (1u << 18) : words;
        if (cap > (uint64_t)SIZE_MAX / sizeof(uint32_t)) return hipErrorOutOfMemory;
        hipError_t e = hipMalloc(&c->eq_ws, (size_t)cap * sizeof(uint32_t));
        if (e != hipSuccess) {  // whatever the runtime calls it: the caller sees NFCS_ENOMEM
            c->eq_ws = nullptr;
            (void)hipGetLastError();
            return hipErrorOutOfMemory;
        }
        c->eq_cap = cap;
    } else if (c->eq_used && c->eq_stream != st) {
        hipError_t e = wait_eq_user(c, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t release_eq(nfcs_ctx* c, hipStream_t st) {
    c->eq_stream = st;
    c->eq_used = true;
    c->eq_own = st == c->stream;
    return c->eq_own ? hipSuccess : hipEventRecord(c->eq_ev, st);
}

// The same for the stage counters' stripes (ct_ws), of one size: allocated and zeroed by the first call that
// counts, on the host, before that call launches anything. A failed allocation leaves the context as it was.
hipError_t acquire_ct(nfcs_ctx* c, hipStream_t st) {
    if (!c->ct_ws) {
        uint64_t* p = nullptr;
        const size_t bytes = (size_t)nfcs::kCtSlots * sizeof(uint64_t);
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return hipErrorOutOfMemory;
        }
        e = hipMemset(p, 0, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();  // the zeros are there whatever stream counts first
        if (e != hipSuccess) {
            (void)hipFree(p);
            return e;
        }
        c->ct_ws = p;
    } else if (c->ct_used && c->ct_stream != st) {
        if (c->ct_own) {
            hipError_t e = hipEventRecord(c->ct_ev, c->stream);
            if (e != hipSuccess) return e;
        }
        return hipStreamWaitEvent(st, c->ct_ev, 0);
    }
    return hipSuccess;
}
hipError_t release_ct(nfcs_ctx* c, hipStream_t st) {
    c->ct_stream = st;
    c->ct_used = true;
    c->ct_own = st == c->stream;
    return c->ct_own ? hipSuccess : hipEventRecord(c->ct_ev, st);
}

int hip_fail(hipError_t e) {
    g_last_hip = (int)e;
    return NFCS_EHIP;
}
#define NFCS_HIP(x)                              \
    do {                                         \
        hipError_t e_ = (x);                     \
        if (e_ != hipSuccess) return hip_fail(e_); \
    } while (0)

hipStream_t pick(nfcs_ctx* ctx, void* s) { return s ? (hipStream_t)s : ctx->stream; }

// Makes `device` current on the calling thread for one entry point and restores the caller's
// device on return: a context may be driven from any host thread (netflow_amd::MultiGpu runs one
// thread per GPU), and allocations / copies must land on the context's device.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) err = hipSetDevice(device);
        else prev = -1;  // nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// The GPU's NUMA node from sysfs (PCI bus id -> /sys/bus/pci/devices/<id>/numa_node), -1 if unknown.
int gpu_numa_node(int device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    for (char* q = bus; *q; ++q) *q = (char)((*q >= 'A' && *q <= 'F') ? *q - 'A' + 'a' : *q);
    char path[160];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

// The CPUs of a NUMA node (/sys/devices/system/node/node<N>/cpulist, e.g. "0-31,128-159").
bool node_cpus(int node, cpu_set_t* set) {
    char path[96];
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    FILE* f = fopen(path, "r");
    if (!f) return false;
    char buf[4096] = {0};
    const bool ok = fgets(buf, sizeof(buf), f) != nullptr;
    fclose(f);
    if (!ok) return false;
    CPU_ZERO(set);
    int n = 0;
    for (char* q = buf; *q && *q != '\n';) {
        char* e;
        const long a = strtol(q, &e, 10);
        if (e == q) break;
        long b = a;
        if (*e == '-') b = strtol(e + 1, &e, 10);
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c, ++n) CPU_SET((int)c, set);
        q = (*e == ',') ? e + 1 : e;
    }
    return n > 0;
}

hipError_t host_block_alloc(HostBlock& b, size_t bytes, int node, bool* local) {
    b.bytes = bytes;
    *local = false;
    if (node >= 0 && node < 1024) {
        void* p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p != MAP_FAILED) {
            unsigned long mask[16] = {0};
            mask[node / 64] |= 1ul << (node % 64);
            // MPOL_PREFERRED (1): the node's memory while it has free pages, never a failure
            const bool bound = syscall(SYS_mbind, p, bytes, 1, mask, 16 * 64 + 1, 0) == 0;
            memset(p, 0, bytes);  // fault the pages in on the node
            if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) {
                b.p = p;
                b.mapped = true;
                *local = bound;
                return hipSuccess;
            }
            (void)hipGetLastError();
            munmap(p, bytes);
        }
    }
    return hipHostMalloc(&b.p, bytes, hipHostMallocDefault);
}

void host_block_free(HostBlock& b) {
    if (!b.p) return;
    if (b.mapped) {
        (void)hipHostUnregister(b.p);
        munmap(b.p, b.bytes);
    } else {
        (void)hipHostFree(b.p);
    }
    b = HostBlock{};
}

// A pointer into slot s's pinned block, as the GPU addresses it.
template <class T>
T* zdev(const nfcs_ctx* c, int s, T* host) {
    return host ? reinterpret_cast<T*>(c->z_block[s] + (reinterpret_cast<const uint8_t*>(host) -
                                                        static_cast<const uint8_t*>(c->hb[s].p)))
                : nullptr;
}

// Direct chunks (round 6, VERDICT r5 item 2: the per-RX-burst operating point). A chunk of at most
// kDirectChunkBytes of frames moves no DMA at all: the kernel reads its descriptors and frames where
// the host left them (the slot's pinned block, or a pinned caller arena in place) and writes its patch
// records and statuses straight into the slot's pinned block; the host waits for one event. At these
// sizes a call is bound by fixed costs, and the three copy-engine transfers it saves (descriptors,
// frames in, records out: each a queued DMA with its own setup latency) were most of them: 256 C1
// frames through nfcs_update_host 49.5 µs per call with copies, 26.4 in the zero-copy form
// (profiles/r06_host_bursts_*.json). Larger chunks keep the copy engines, which move bytes over PCIe
// faster than kernel loads do (1M C1 frames: 51.7 against 43 GB/s zero-copy).
#ifndef NFCS_DIRECT_CHUNK_BYTES
#define NFCS_DIRECT_CHUNK_BYTES (2u << 20)
#endif
constexpr uint64_t kDirectChunkBytes = NFCS_DIRECT_CHUNK_BYTES;
constexpr uint64_t kZeroCopyAutoBytes = NFCS_HOST_ZERO_COPY_AUTO_BYTES;  // nfcs.h
// The staged chunk size of a host burst of `total` bytes: about total / kChunksPerBurst (at least
// kMinChunkBytes, at most a staging slot), so that the host copies, the transfers, the kernel and the
// write-back of successive chunks overlap across the two slots even when the burst would fit one slot
// (round 2: 16K C1 frames pinned 583 -> 559 µs, pageable 979 -> 710 µs in 4 chunks of >= 4 MiB).
#ifndef NFCS_MIN_CHUNK_BYTES
#define NFCS_MIN_CHUNK_BYTES (4ull << 20)
#endif
#ifndef NFCS_CHUNKS_PER_BURST
#define NFCS_CHUNKS_PER_BURST 4
#endif
constexpr uint64_t kMinChunkBytes = NFCS_MIN_CHUNK_BYTES;
constexpr uint64_t kChunksPerBurst = NFCS_CHUNKS_PER_BURST;
inline uint64_t chunk_bytes(uint64_t total) {
    return std::min<uint64_t>(nfcs_ctx::kStageBytes, std::max<uint64_t>(kMinChunkBytes, total / kChunksPerBurst));
}
// Host copy work per thread before a copy is split over the workers (a worker's wake-up costs ~10 µs;
// one thread stages ~15 GB/s): gathers and staging copies from 512 KiB, write-backs from 2048 frames.
#ifndef NFCS_COPY_BYTES_PER_THREAD
#define NFCS_COPY_BYTES_PER_THREAD (512u << 10)
#endif
constexpr uint64_t kCopyBytesPerThread = NFCS_COPY_BYTES_PER_THREAD;
constexpr uint32_t kPatchFramesPerThread = 2048;

// Host copies whose destination this CPU does not read again (the staging slots, which the copy
// engine reads next; frames copied back into a caller's arena): 16-byte non-temporal stores, so a
// destination line is written once instead of first being read for ownership (a plain memcpy of a
// 1500-byte frame moves 3 bytes over the memory bus per byte copied, this 2). Bytes before dst's
// first 16-byte boundary and after its last go through plain stores; with zero_pad the last partial
// chunk is instead stored whole, its bytes past len zeroed (the staged frames' 16-byte padding, which
// the kernels read). Every worker that streamed calls nt_fence() before its part counts as done.
typedef uint32_t host_u32x4 __attribute__((ext_vector_type(4)));
static inline void stream_copy(uint8_t* dst, const uint8_t* src, uint64_t len, bool zero_pad) {
    uint64_t k = std::min<uint64_t>(len, (16u - ((uintptr_t)dst & 15u)) & 15u);
    if (k) memcpy(dst, src, k);
    for (; k + 64 <= len; k += 64) {
        host_u32x4 a, b, c, d;
        memcpy(&a, src + k, 16); memcpy(&b, src + k + 16, 16);
        memcpy(&c, src + k + 32, 16); memcpy(&d, src + k + 48, 16);
        __builtin_nontemporal_store(a, (host_u32x4*)(dst + k));
        __builtin_nontemporal_store(b, (host_u32x4*)(dst + k + 16));
        __builtin_nontemporal_store(c, (host_u32x4*)(dst + k + 32));
        __builtin_nontemporal_store(d, (host_u32x4*)(dst + k + 48));
    }
    for (; k + 16 <= len; k += 16) {
        host_u32x4 a;
        memcpy(&a, src + k, 16);
        __builtin_nontemporal_store(a, (host_u32x4*)(dst + k));
    }
    if (k < len) {
        if (zero_pad && !((uintptr_t)(dst + k) & 15u)) {
            host_u32x4 t = {0u, 0u, 0u, 0u};
            memcpy(&t, src + k, len - k);
            __builtin_nontemporal_store(t, (host_u32x4*)(dst + k));
        } else {
            memcpy(dst + k, src + k, len - k);
        }
    }
}
static inline void nt_fence() { __builtin_ia32_sfence(); }  // the non-temporal stores drained

// Copy split across the context's workers: one host thread copies pageable memory at ~15-25 GB/s,
// below what PCIe moves (e2e: pageable staging 27 GB/s single-threaded vs 54 GB/s pinned). The
// workers run on the GPU's NUMA node, next to the staging memory.
void par_memcpy(nfcs_ctx* c, void* dst, const void* src, size_t bytes) {
    const size_t kMin = kCopyBytesPerThread;
    if (bytes < 2 * kMin || c->workers.size() == 0) {
        stream_copy((uint8_t*)dst, (const uint8_t*)src, bytes, false);
        nt_fence();
        return;
    }
    const size_t t = std::min<size_t>((size_t)c->workers.size() + 1, bytes / kMin);
    const size_t per = (bytes / t + 4095) & ~size_t(4095);
    c->workers.run((int)t, [&](int i) {
        const size_t o = (size_t)i * per;
        if (o < bytes) stream_copy((uint8_t*)dst + o, (const uint8_t*)src + o, std::min(per, bytes - o), false);
        nt_fence();
    });
}

// Frees the host pipeline's streams, events and buffers (also a partly built one).
void free_host_pipeline(nfcs_ctx* c) {
    c->host_ready = false;
    c->workers.stop();
    if (c->done_host) {
        for (int s = 0; s < nfcs_ctx::kSlots; ++s)
            if (c->hs[s]) (void)hipStreamSynchronize(c->hs[s]);  // no launch still counting into them
        (void)hipHostFree(c->done_host);
    }
    if (c->done_ctr) (void)hipFree(c->done_ctr);
    c->done_host = nullptr;
    c->done_dev = nullptr;
    c->done_ctr = nullptr;
    for (int s = 0; s < nfcs_ctx::kSlots; ++s) {
        if (c->hs[s]) { (void)hipStreamSynchronize(c->hs[s]); (void)hipStreamDestroy(c->hs[s]); }
        if (c->done[s]) (void)hipEventDestroy(c->done[s]);
        if (c->staged[s]) (void)hipEventDestroy(c->staged[s]);
        (void)hipFree(c->d_arena[s]);
        (void)hipFree(c->d_desc[s]);
        (void)hipFree(c->d_status[s]);
        (void)hipFree(c->d_patch[s]);
        host_block_free(c->hb[s]);
        c->hs[s] = nullptr;
        c->done[s] = nullptr;
        c->staged[s] = nullptr;
        c->d_arena[s] = nullptr;
        c->d_desc[s] = nullptr;
        c->d_status[s] = nullptr;
        c->d_patch[s] = nullptr;
        c->h_arena[s] = nullptr;
        c->z_block[s] = nullptr;
        c->h_desc[s] = nullptr;
        c->h_status[s] = nullptr;
        c->h_patch[s] = nullptr;
    }
}

int build_host_pipeline(nfcs_ctx* ctx);

// A direct chunk's completion request for slot s (nfcs::DoneReq), or none where the context has no flags.
nfcs::DoneReq done_req(nfcs_ctx* c, int s) {
    c->slot_wait[s] = c->done_host ? 1 : 0;
    if (!c->done_host) return {};
    return {c->done_dev + 8 * s, c->done_ctr + s, c->done_base[s]};
}
// The chunk launched in slot s is waited for on its events.
void event_wait(nfcs_ctx* c, int s) { c->slot_wait[s] = 0; }

// Waits for the chunk in slot s: on its completion flag when it has one (a direct chunk: the kernel's
// last workgroup publishes the count; once seen, later waits for the same chunk return at once), else
// — or after kFlagSpinNs without the flag, e.g. a launch that failed — on the event.
hipError_t wait_slot(nfcs_ctx* c, int s, hipEvent_t ev) {
    constexpr int64_t kFlagSpinNs = 20000000;
    if (c->slot_wait[s] == 2) return hipSuccess;
    if (c->slot_wait[s] == 1) {
        const uint64_t base = c->done_base[s];
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t k = 1;; ++k) {
            const uint64_t v = __atomic_load_n(c->done_host + 8 * s, __ATOMIC_ACQUIRE);
            if (v > base) {
                c->done_base[s] = v;
                c->slot_wait[s] = 2;
                return hipSuccess;
            }
            if ((k & 1023u) == 0 &&
                std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() > kFlagSpinNs)
                break;
            __builtin_ia32_pause();
        }
        const hipError_t e = hipEventSynchronize(ev);
        c->done_base[s] = std::max(c->done_base[s], __atomic_load_n(c->done_host + 8 * s, __ATOMIC_ACQUIRE));
        c->slot_wait[s] = 0;
        return e;
    }
    return hipEventSynchronize(ev);
}

// The host pipeline, built on first use on the context's device (the caller holds a DeviceGuard).
// A build that fails part-way is torn down, so the next call retries it instead of using half of it.
int ensure_host_pipeline(nfcs_ctx* ctx) {
    if (ctx->host_ready) return NFCS_OK;
    const int rc = build_host_pipeline(ctx);
    if (rc != NFCS_OK) {
        free_host_pipeline(ctx);
        return rc;
    }
    ctx->host_ready = true;
    return NFCS_OK;
}

int build_host_pipeline(nfcs_ctx* ctx) {
    // host threads for the staging copies, gathers and write-back: 8, or NFCS_HOST_THREADS (1-64) —
    // a caller that shares the host's cores with other work, or has more to give, sets it
    ctx->copy_threads = 8;
    if (const char* e = getenv("NFCS_HOST_THREADS")) {
        const int t = atoi(e);
        if (t >= 1 && t <= 64) ctx->copy_threads = t;
    }
    ctx->stage_bytes = nfcs_ctx::kStageBytes;
    ctx->stage_pkts = (uint32_t)(ctx->stage_bytes / 64);
    // staging ring on the GPU's NUMA node, copy threads on its CPUs
    ctx->numa_node = gpu_numa_node(ctx->di.device);
    ctx->have_cpus = ctx->numa_node >= 0 && node_cpus(ctx->numa_node, &ctx->node_cpus);
    const size_t a_desc = (size_t)ctx->stage_pkts * sizeof(nfcs_desc);
    const size_t a_patch = (size_t)ctx->stage_pkts * sizeof(nfcs_patch);
    const size_t a_status = ((size_t)ctx->stage_pkts + 4095) & ~size_t(4095);
    bool local = true;
    for (int s = 0; s < nfcs_ctx::kSlots; ++s) {
        NFCS_HIP(hipStreamCreateWithFlags(&ctx->hs[s], hipStreamNonBlocking));
        NFCS_HIP(hipEventCreateWithFlags(&ctx->done[s], hipEventDisableTiming));
        NFCS_HIP(hipEventCreateWithFlags(&ctx->staged[s], hipEventDisableTiming));
        NFCS_HIP(hipMalloc(&ctx->d_arena[s], ctx->stage_bytes));
        NFCS_HIP(hipMalloc(&ctx->d_desc[s], a_desc));
        NFCS_HIP(hipMalloc(&ctx->d_status[s], ctx->stage_pkts));
        NFCS_HIP(hipMalloc(&ctx->d_patch[s], a_patch));
        // one pinned block per slot: arena | descriptors | patch records | statuses
        bool l = false;
        NFCS_HIP(host_block_alloc(ctx->hb[s], ctx->stage_bytes + a_desc + a_patch + a_status,
                                  ctx->numa_node, &l));
        local = local && l;
        uint8_t* p = static_cast<uint8_t*>(ctx->hb[s].p);
        ctx->h_arena[s] = p;
        ctx->h_desc[s] = reinterpret_cast<nfcs_desc*>(p + ctx->stage_bytes);
        ctx->h_patch[s] = reinterpret_cast<nfcs_patch*>(p + ctx->stage_bytes + a_desc);
        ctx->h_status[s] = p + ctx->stage_bytes + a_desc + a_patch;
        // the block as the GPU addresses it (registered and hipHostMalloc'd memory is mapped): direct
        // chunks read their frames and descriptors and write their records and statuses here
        void* zp = nullptr;
        if (hipHostGetDevicePointer(&zp, p, 0) == hipSuccess) ctx->z_block[s] = static_cast<uint8_t*>(zp);
        else (void)hipGetLastError();
    }
    ctx->numa_local = local;
    // completion flags of direct chunks: optional (without them the chunks wait on their events)
    if (hipHostMalloc((void**)&ctx->done_host, nfcs_ctx::kSlots * 64, hipHostMallocMapped) == hipSuccess &&
        hipHostGetDevicePointer((void**)&ctx->done_dev, ctx->done_host, 0) == hipSuccess &&
        hipMalloc((void**)&ctx->done_ctr, nfcs_ctx::kSlots * sizeof(uint64_t)) == hipSuccess &&
        hipMemset(ctx->done_ctr, 0, nfcs_ctx::kSlots * sizeof(uint64_t)) == hipSuccess) {
        memset(ctx->done_host, 0, nfcs_ctx::kSlots * 64);
    } else {
        (void)hipGetLastError();
        if (ctx->done_host) (void)hipHostFree(ctx->done_host);
        if (ctx->done_ctr) (void)hipFree(ctx->done_ctr);
        ctx->done_host = nullptr;
        ctx->done_dev = nullptr;
        ctx->done_ctr = nullptr;
    }
    for (int s = 0; s < nfcs_ctx::kSlots; ++s) {
        ctx->done_base[s] = 0;
        ctx->slot_wait[s] = 0;
    }
    ctx->workers.start(ctx->copy_threads - 1, ctx->have_cpus ? &ctx->node_cpus : nullptr);
    return NFCS_OK;
}

bool is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// A caller's descriptor as the host path stages it: a frame inside the arena that is longer than
// kFrameRelevantBytes goes as its first kFrameRelevantBytes — the same result (nfcs.h), and no frame
// outgrows a staging slot; others unchanged (a frame reaching past the arena stays NFCS_ST_BAD_DESC).
inline nfcs_desc staged_desc(const nfcs_desc& d, uint64_t arena_bytes) {
    const uint64_t o = (uint64_t)d.off16 * 16u;
    if (d.len > nfcs::kFrameRelevantBytes && o + (((uint64_t)d.len + 15u) & ~15ull) <= arena_bytes)
        return nfcs_desc{d.off16, nfcs::kFrameRelevantBytes};
    return d;
}
// Descriptors [i, i + m) into a staging slot, as staged_desc stages them (a plain copy when the burst
// has no frame longer than kFrameRelevantBytes).
void stage_descs(nfcs_desc* dst, const nfcs_desc* src, uint32_t m, uint64_t arena_bytes, bool any_long) {
    if (!any_long) {
        memcpy(dst, src, (size_t)m * sizeof(nfcs_desc));
        return;
    }
    for (uint32_t j = 0; j < m; ++j) dst[j] = staged_desc(src[j], arena_bytes);
}

// The arena bytes that descriptors [i0, i1) span, summed over their runs of ascending offsets: a NIC
// ring burst that wraps past the ring's end is two runs, each from its first frame's start to the end
// of its furthest frame (frames outside the arena count nothing). The launch shape's footprint.
uint64_t run_span(const nfcs_desc* d, uint32_t i0, uint32_t i1, uint64_t arena_bytes) {
    uint64_t total = 0, lo = 0, hi = 0;
    for (uint32_t i = i0; i < i1; ++i) {
        const nfcs_desc sd = staged_desc(d[i], arena_bytes);
        const uint64_t o = (uint64_t)sd.off16 * 16u, e = o + (((uint64_t)sd.len + 15u) & ~15ull);
        if (i == i0 || d[i].off16 < d[i - 1].off16) {  // a new run
            total += hi - lo;
            lo = hi = std::min(o, arena_bytes);
        }
        if (e <= arena_bytes) hi = std::max(hi, e);
    }
    return total + (hi - lo);
}

// Pinned host arena: the kernel reads the frames over PCIe where they are and writes the 2+2
// checksum bytes straight back (host memory from hipHostMalloc is mapped into the GPU's address
// space), inline from the read pass (kUpdateInline: a deferred write pass would cross the link
// again). The descriptors (8 B/packet) are copied into a staging slot's pinned block, where the kernel
// reads them, and the statuses (1 B/packet) come back there (round 6; copied H2D / D2H by DMA before),
// in chunks on the two pipeline streams; frames cross the link once, in one direction. On an error both
// slots are drained before returning, so nothing is left in flight on the caller's memory. Also the
// default form of nfcs_update_host for pinned bursts of up to kZeroCopyAutoBytes.
int update_host_zero_copy(nfcs_ctx* c, uint8_t* h_arena, uint64_t arena_bytes,
                          const nfcs_desc* h_desc, uint32_t n, uint8_t* h_status, bool any_long) {
    void* dptr = nullptr;
    NFCS_HIP(hipHostGetDevicePointer(&dptr, h_arena, 0));
    uint8_t* d_arena = static_cast<uint8_t*>(dptr);
    uint32_t cnt[nfcs_ctx::kSlots] = {0, 0}, first[nfcs_ctx::kSlots] = {0, 0};
    hipError_t e = hipSuccess;
    // wait for slot s; its statuses are copied out only while no error has occurred
    auto finish = [&](int s) {
        if (!cnt[s]) return;
        const hipError_t f = wait_slot(c, s, c->done[s]);
        if (e == hipSuccess) e = f;
        if (e == hipSuccess && h_status) memcpy(h_status + first[s], c->h_status[s], cnt[s]);
        cnt[s] = 0;
    };
    int s = 0;
    for (uint32_t i = 0; i < n && e == hipSuccess; s ^= 1) {
        finish(s);
        if (e != hipSuccess) break;
        const uint32_t m = std::min<uint32_t>(n - i, c->stage_pkts);
        hipStream_t st = c->hs[s];
        stage_descs(c->h_desc[s], h_desc + i, m, arena_bytes, any_long);
        // the launch shape follows this chunk's own frames (their span per packet, over the runs of
        // a burst that wraps its ring), not the caller's whole arena, unless the context has a hint
        const uint64_t span = run_span(h_desc, i, i + m, arena_bytes);
        uint64_t shape = c->slot_bytes;
        if (!shape) shape = std::max<uint64_t>(1, span / m);
        if (c->z_block[s]) {
            // round 6: the kernel reads the chunk's descriptors from the slot's pinned block and writes
            // its statuses there (no DMA at all: burst sizes where the call is bound by fixed costs); a
            // small chunk signals its completion through the slot's flag (nfcs::DoneReq)
            const nfcs::DoneReq dr = span <= kDirectChunkBytes ? done_req(c, s) : nfcs::DoneReq{};
            if (!dr.flag) event_wait(c, s);
            e = nfcs::launch_update(c->di, d_arena, arena_bytes, zdev(c, s, c->h_desc[s]), m, 0u,
                                    h_status ? zdev(c, s, c->h_status[s]) : nullptr, nullptr, nullptr,
                                    nfcs::kUpdateInline, st, shape, {}, dr);
        } else {
            event_wait(c, s);
            e = hipMemcpyAsync(c->d_desc[s], c->h_desc[s], (size_t)m * sizeof(nfcs_desc),
                               hipMemcpyHostToDevice, st);
            if (e == hipSuccess)
                e = nfcs::launch_update(c->di, d_arena, arena_bytes, c->d_desc[s], m, 0u,
                                        h_status ? c->d_status[s] : nullptr, nullptr, nullptr,
                                        nfcs::kUpdateInline, st, shape);
            if (e == hipSuccess && h_status)
                e = hipMemcpyAsync(c->h_status[s], c->d_status[s], m, hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess) e = hipEventRecord(c->done[s], st);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);  // whatever was queued on this slot has finished
            break;
        }
        first[s] = i;
        cnt[s] = m;
        i += m;
    }
    finish(s);  // drain both slots, also after an error
    finish(s ^ 1);
    if (e != hipSuccess) return hip_fail(e);
    return NFCS_OK;
}

// The launch shape's mean footprint per packet for a device call (speed only; the bytes written
// never depend on it): the context's slot-size hint when set; else arena_bytes / n, which is exact
// for a batch that fills its arena and can only over-estimate (frames never overlap). So a short
// estimate is right, and only a long one can be wrong — a burst inside a larger ring. Then the call
// also has its launch sample the frames' real footprint (sample_footprint, one wave, host-mapped
// result), and the next call on the same burst (descriptor array, n and arena_bytes; up to kObsSlots
// bursts tracked, least recently used replaced) launches in the shape that sample says: a NIC ring
// reusing its descriptor arrays adapts after one call, with no hint and no host sync.
struct Shape { uint64_t mean; nfcs::ObsReq obs; uint32_t bits = 0; };  // bits: the sample's kObsUnaligned / kObsMixed
// The burst's observation slot, or -1 (no side effects).
int find_burst(const nfcs_ctx* c, uint64_t arena_bytes, const nfcs_desc* d_desc, uint32_t n) {
    for (int k = 0; k < nfcs_ctx::kObsSlots; ++k) {
        const nfcs_ctx::ObsBurst& b = c->obs_burst[k];
        if (b.gen && b.desc == d_desc && b.n == n && b.bytes == arena_bytes) return k;
    }
    return -1;
}
// The shape a call over this burst launches in, without side effects (nfcs_ctx_launch_footprint):
// *slot = the burst's observation slot, -1 when it has none yet (the call then takes one).
// Estimates that a sample can correct: "long" (a burst inside a larger ring), and "8-lane rows" (a
// densely packed mix whose frames often need a second 8-lane row pass; round 6).
// (the forward samples mid-size estimates too: ShapeRule::packed_rows8)
bool sampled_estimate(uint64_t est, bool mid = false) {
    return mid || est >= nfcs::kSmallMeanBytes || est < nfcs::kTinyMeanBytes;
}
// Each op's use of the sample (nfcs_internal.h, after kTinyMixMeanBytes): the mean from which a mix with
// many long frames leaves 8-lane rows, whether mid-size frames of one length in a ring take 8-lane rows,
// whether a mix with hardly any mid-length frames (64 / 1500-byte traffic) stays on them, and whether
// densely packed mid-size frames of one length on their own lines take them too (sampled for it).
struct ShapeRule { uint64_t mix_mean; bool ring_rows8; bool bimodal_rows8; bool packed_rows8; };
constexpr ShapeRule kUpdateRule = {nfcs::kTinyMixMeanBytes, true, false, false};
constexpr ShapeRule kFwdRule = {nfcs::kTinyMixMeanBytes, true, true, true};
constexpr ShapeRule kVlanRule = {nfcs::kVlanMixMeanBytes, false, false, false};
Shape peek_shape(const nfcs_ctx* c, uint64_t arena_bytes, const nfcs_desc* d_desc, uint32_t n, int* slot,
                 const ShapeRule& rule = kUpdateRule) {
    *slot = -1;
    if (c->slot_bytes) return {c->slot_bytes, {}};
    if (n == 0) return {arena_bytes, {}};  // nothing is launched; never divide by zero
    const uint64_t est = arena_bytes / n;
    if (!sampled_estimate(est, rule.packed_rows8) || !c->obs_host) return {est, {}};
    const int k = find_burst(c, arena_bytes, d_desc, n);
    if (k < 0) return {est, {}};
    *slot = k;
    // the latest sample of this burst's generation (a late one of an earlier burst has another)
    const uint64_t o = __atomic_load_n(c->obs_host + k, __ATOMIC_RELAXED);
    const uint32_t gen = c->obs_burst[k].gen;
    const nfcs::ObsReq req = {c->obs_dev + k, ((uint64_t)gen << 32) | n};
    if ((uint32_t)(o >> 32) != gen || !((uint32_t)o & nfcs::kObsPresent)) return {est, req};
    uint64_t mean = std::min<uint64_t>((uint32_t)o & nfcs::kObsMeanMask, est);
    // 8-lane rows only for frames that mostly fit their one row pass, or short enough on average that
    // the packet rate bounds them (nfcs_internal.h kTinyLongMax, kTinyMixMeanBytes), or — the forward —
    // a mix of short and full-size frames with hardly any in between (kObsMidShift)
    const bool bimodal = rule.bimodal_rows8 && (((uint32_t)o >> nfcs::kObsMidShift) & 7u) < nfcs::kObsMidMin8;
    if (mean < nfcs::kTinyMeanBytes && mean >= rule.mix_mean && !bimodal &&
        (((uint32_t)o >> nfcs::kObsLongShift) & 0x1FFu) > nfcs::kTinyLongMax)
        mean = nfcs::kTinyMeanBytes;
    const uint32_t bits = (uint32_t)o & (nfcs::kObsUnaligned | nfcs::kObsMixed);
    // a ring (the sample corrected a "long" estimate) of mid-size frames of one length, each on its own
    // lines — or, for the forward, such frames packed: 8-lane rows (nfcs_internal.h, after
    // kTinyMixMeanBytes)
    if (rule.ring_rows8 && !bits && (est >= nfcs::kSmallMeanBytes || rule.packed_rows8) &&
        mean >= nfcs::kTinyMeanBytes && mean < nfcs::kSmallMeanBytes)
        mean = nfcs::kTinyMeanBytes - 1;
    return {mean, req, bits};
}
Shape launch_shape(nfcs_ctx* c, uint64_t arena_bytes, const nfcs_desc* d_desc, uint32_t n,
                   const ShapeRule& rule = kUpdateRule) {
    int k = -1;
    Shape sh = peek_shape(c, arena_bytes, d_desc, n, &k, rule);
    if (sh.obs.slot == nullptr && k < 0 && !c->slot_bytes && n && c->obs_host &&
        sampled_estimate(arena_bytes / n, rule.packed_rows8)) {
        // a burst not seen lately: the least recently used slot, under a new generation
        k = 0;
        for (int j = 1; j < nfcs_ctx::kObsSlots; ++j)
            if (c->obs_burst[j].used < c->obs_burst[k].used) k = j;
        if (++c->obs_gen == 0) c->obs_gen = 1;
        c->obs_burst[k] = {d_desc, n, arena_bytes, c->obs_gen, 0};
        sh.obs = {c->obs_dev + k, ((uint64_t)c->obs_gen << 32) | n};
    }
    if (k >= 0) c->obs_burst[k].used = ++c->obs_clock;
    return sh;
}

// The device-resident update on stream st: kUpdateAuto, deferred records into the caller's
// d_patch when given, else into the context workspace.
// The newest store-demand observation the device has forwarded, fed to the policy (no sync: a word the
// device writes with one 64-bit store; a generation the context no longer remembers is skipped).
void read_store_demand(nfcs_ctx* c) {
    if (!c->dem_host) return;
    const uint64_t o = __atomic_load_n(c->dem_host, __ATOMIC_RELAXED);
    const uint32_t gen = (uint32_t)(o >> 32);
    if (!c->dem_policy.newer(gen)) return;
    const nfcs_ctx::DemCall& dc = c->dem_calls[gen % nfcs_ctx::kDemRing];
    if (dc.gen == gen) c->dem_policy.observe(gen, dc.sampled, (uint32_t)o);
}

// A long-shape call of more than kInlineMaxPackets packets runs deferred (sub-batches of a read pass
// writing records and a write pass) or sparse (one inline launch), by the context's policy over the store
// demand of its last calls (nfcs_store_policy.h). Speed only: bytes, status bytes and
// records never depend on the form. A caller's d_patch keeps the call deferred (its records hold every
// field); a call on another stream than the previous update call's returns the context to deferred, since
// calls that may run concurrently share the counters.
int update_device(nfcs_ctx* c, uint8_t* d_arena, uint64_t arena_bytes, const nfcs_desc* d_desc,
                  uint32_t n, uint8_t* d_status, nfcs_patch* d_patch, hipStream_t st) {
    if (!d_patch) NFCS_HIP(acquire_ws(c, n, st));
    const Shape sh = launch_shape(c, arena_bytes, d_desc, n);
    nfcs::DemandReq dem;
    bool sparse = false;
    const bool changed = c->dem_any && c->dem_stream != st;
    c->dem_stream = st;
    c->dem_any = true;
    c->dem_last_form = 0;
    // the next two counting calls use buffers that a call still running on the other stream may be
    // forwarding or counting into: their observations are skipped
    if (changed) c->dem_policy.reset(c->dem_gen + 2u);
    if (c->dem_dev && nfcs::update_demand_sampled(arena_bytes, n, sh.mean, false)) {
        read_store_demand(c);
        if (!d_patch)
            sparse = c->store_policy == NFCS_STORE_SPARSE ||
                     (c->store_policy == NFCS_STORE_AUTO && c->dem_policy.form == nfcs::kStoreFormSparse);
        const uint32_t prev = c->dem_gen;
        if (++c->dem_gen == 0) c->dem_gen = 1;
        const uint32_t words = nfcs::kDemandWords * nfcs::kDemandStrideWords;
        c->dem_calls[c->dem_gen % nfcs_ctx::kDemRing] = {c->dem_gen,
                                                         nfcs::update_demand_sampled(arena_bytes, n, sh.mean, sparse)};
        dem.cur = c->dem_dev + (c->dem_gen & 1u) * words;
        dem.prev = c->dem_dev + (prev & 1u) * words;
        dem.host = prev ? c->dem_host_dev : nullptr;
        dem.prev_gen = prev;
        if (prev && (prev & 1u) == (c->dem_gen & 1u)) dem.host = nullptr;  // the generation wrapped past 0
        c->dem_last_form = sparse ? NFCS_STORE_SPARSE : NFCS_STORE_DEFERRED;
    }
    NFCS_HIP(nfcs::launch_update(c->di, d_arena, arena_bytes, d_desc, n, 0u, d_status, d_patch,
                                 d_patch ? nullptr : c->ws, nfcs::kUpdateAuto, st, sh.mean, sh.obs, {}, dem, sparse));
    if (!d_patch) NFCS_HIP(release_ws(c, st));
    return NFCS_OK;
}

// The fused L3 forward on stream st; a burst above kFwdDeferAbovePackets defers the stores of its
// long-frame waves through forward records in the context workspace (one per packet of a sub-batch).
int l3_forward_device(nfcs_ctx* c, uint8_t* d_arena, uint64_t arena_bytes, const nfcs_desc* d_desc,
                      const uint32_t* d_nh, uint32_t n, const nfcs_nexthop* d_table, uint32_t table_n,
                      uint8_t* d_status, hipStream_t st) {
    const bool dfr = n > nfcs::kFwdDeferAbovePackets;
    if (dfr) NFCS_HIP(acquire_ws(c, nfcs::kSubBatchPackets, st));
    const Shape sh = launch_shape(c, arena_bytes, d_desc, n, kFwdRule);
    NFCS_HIP(nfcs::launch_l3_forward(c->di, d_arena, arena_bytes, d_desc, d_nh, n, d_table, table_n,
                                     d_status, dfr ? c->ws : nullptr, st, sh.mean, sh.obs));
    if (dfr) NFCS_HIP(release_ws(c, st));
    return NFCS_OK;
}

// ---- the life cycle the six table objects share -------------------------------------
// Setters change `in` and clear `committed`; commit compiles `in` into `t`; upload snapshots `t` into one
// device allocation on `device`, which nothing but the next upload or the destroy changes.
template <class In, class Tables, class Dev>
struct Table {
    In in;
    Tables t;
    bool committed = false;
    int device = -1;
    uint8_t* d_blob = nullptr;
    Dev dev{};
    bool uploaded = false;
    void drop_upload() {
        if (d_blob) {
            DeviceGuard dg_(device);
            if (dg_.err == hipSuccess) (void)hipFree(d_blob);
        }
        d_blob = nullptr;
        dev = Dev{};
        uploaded = false;
    }
};

template <class T>
int table_create(T** out) {
    if (!out) return NFCS_EINVAL;
    *out = new (std::nothrow) T();
    return *out ? NFCS_OK : NFCS_ENOMEM;
}
template <class T>
int table_destroy(T* t) {
    if (!t) return NFCS_EINVAL;
    t->drop_upload();
    delete t;
    return NFCS_OK;
}

// fn() as a return code: NFCS_OK for one that returns nothing, NFCS_ENOMEM for one that throws.
template <class F>
int guarded(F&& fn) {
    try {
        if constexpr (std::is_void_v<decltype(fn())>) {
            fn();
            return NFCS_OK;
        } else {
            return fn();
        }
    } catch (...) {
        return NFCS_ENOMEM;
    }
}
// A setter's change to t->in. A rejected one leaves the commit standing; after an accepted one the object is
// uncommitted, and the device copy, if any, stays as it is until the next upload.
template <class T, class F>
int table_set(T* t, F&& fn) {
    if (!t) return NFCS_EINVAL;
    const int rc = guarded(fn);
    if (rc == NFCS_OK) t->committed = false;
    return rc;
}
// The setters that replace one input array.
template <class T, class In, class V>
int table_assign(T* t, std::vector<V> In::*field, const V* src, uint32_t n) {
    if (!t || (n > 0 && !src)) return NFCS_EINVAL;
    return table_set(t, [&] { (t->in.*field).assign(src, src + n); });
}
// compile(in, t): a table whose compile fails is uncommitted, since t may be half rebuilt.
template <class T, class F>
int table_commit(T* t, F&& compile) {
    if (!t) return NFCS_EINVAL;
    t->committed = false;
    const int rc = guarded([&] { return compile(t->in, t->t); });
    t->committed = rc == NFCS_OK;
    return rc;
}
// A table the device entry points of context c may read.
template <class T>
bool usable(const nfcs_ctx* c, const T* t) {
    return c && t && t->uploaded && t->device == c->di.device;
}

// One device allocation of several arrays, each on a 16-byte boundary, zero between and 16 bytes past them.
struct BlobLayout {
    static constexpr int kMaxParts = 8;
    struct Part { const void* src; size_t bytes, off; };
    Part parts[kMaxParts];
    int n = 0;
    size_t total = 0;
    // Appends `bytes` bytes, copied from src where it is given (zero otherwise); returns their offset.
    size_t part(const void* src, size_t bytes) {
        const size_t at = total;
        if (n < kMaxParts) parts[n] = {src, bytes, at};
        ++n;
        total += (bytes + 15u) & ~(size_t)15u;
        return at;
    }
    template <class V>
    size_t part(const std::vector<V>& v) { return part(v.data(), v.size() * sizeof(V)); }
    // The caller has the owning device current. On an error *d_blob holds what was allocated, if anything.
    hipError_t upload(uint8_t** d_blob) const {
        if (n > kMaxParts) return hipErrorInvalidValue;
        hipError_t e = hipMalloc(d_blob, total + 16u);
        if (e == hipSuccess) e = hipMemset(*d_blob, 0, total + 16u);
        for (int i = 0; i < n && e == hipSuccess; ++i)
            if (parts[i].src && parts[i].bytes)
                e = hipMemcpy(*d_blob + parts[i].off, parts[i].src, parts[i].bytes, hipMemcpyHostToDevice);
        return e;
    }
};

// Replaces t's device copy by the laid-out blob on c's device; bind(d_blob) fills t->dev from the offsets.
// A failure leaves t without a device copy.
template <class T, class Bind>
int table_upload(nfcs_ctx* c, T* t, const BlobLayout& lay, Bind&& bind) {
    t->drop_upload();
    DeviceGuard dg_(c->di.device);
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    t->device = c->di.device;
    const hipError_t e = lay.upload(&t->d_blob);
    if (e != hipSuccess) {
        t->drop_upload();
        return hip_fail(e);
    }
    bind(t->d_blob);
    t->uploaded = true;
    return NFCS_OK;
}

// launch(scratch) on st with `words` words of the context's enqueue scratch (eq_ws), which the flood and the
// ICMP stages use too. Without the memory the context stays usable: only this call's scratch is missing.
template <class Launch>
int with_eq_scratch(nfcs_ctx* c, uint64_t words, hipStream_t st, Launch&& launch) {
    const hipError_t e = acquire_eq(c, words, st);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return NFCS_ENOMEM;
    }
    NFCS_HIP(e);
    NFCS_HIP(launch(c->eq_ws));
    NFCS_HIP(release_eq(c, st));
    return NFCS_OK;
}

// launch(ct) on st with the counter scratch (ct_ws) where the call counts, with null where it does not.
template <class Launch>
int with_ct_scratch(nfcs_ctx* c, bool counts, hipStream_t st, Launch&& launch) {
    if (!counts) {
        NFCS_HIP(launch((uint64_t*)nullptr));
        return NFCS_OK;
    }
    const hipError_t e = acquire_ct(c, st);
    if (e == hipErrorOutOfMemory) return NFCS_ENOMEM;
    NFCS_HIP(e);
    NFCS_HIP(launch(c->ct_ws));
    NFCS_HIP(release_ct(c, st));
    return NFCS_OK;
}

}  // namespace

extern "C" {

NFCS_API int nfcs_abi_version(void) { return NFCS_ABI_VERSION; }

NFCS_API const char* nfcs_strerror(int err) {
    switch (err) {
    case NFCS_OK: return "ok";
    case NFCS_EINVAL: return "invalid argument";
    case NFCS_EHIP: return "HIP runtime error";
    case NFCS_ENOMEM: return "out of memory";
    case NFCS_ENODEV: return "no gfx950 device";
    default: return "unknown error";
    }
}

NFCS_API int nfcs_last_hip_error(void) { return g_last_hip; }

NFCS_API int nfcs_ctx_create(int device, nfcs_ctx** out) {
    if (!out) return NFCS_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        return NFCS_ENODEV;
    }
    DeviceGuard dg_(device);  // the new context's device while it is set up; the caller's after
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipDeviceProp_t prop;
    NFCS_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return NFCS_ENODEV;
    nfcs_ctx* c = new (std::nothrow) nfcs_ctx();
    if (!c) return NFCS_ENOMEM;
    c->di.device = device;
    c->di.cus = prop.multiProcessorCount;
    strncpy(c->di.arch, prop.gcnArchName, sizeof(c->di.arch) - 1);
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&c->d_digest, sizeof(uint64_t));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ws_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->eq_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ct_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->obs_host, nfcs_ctx::kObsSlots * sizeof(uint64_t), hipHostMallocMapped);
    if (e == hipSuccess) {
        for (int k = 0; k < nfcs_ctx::kObsSlots; ++k) c->obs_host[k] = 0;
        e = hipHostGetDevicePointer((void**)&c->obs_dev, c->obs_host, 0);
    }
    const size_t dem_bytes = 2u * nfcs::kDemandWords * nfcs::kDemandStrideWords * sizeof(uint32_t);
    if (e == hipSuccess) e = hipMalloc((void**)&c->dem_dev, dem_bytes);
    if (e == hipSuccess) e = hipMemset(c->dem_dev, 0, dem_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->dem_host, sizeof(uint64_t), hipHostMallocMapped);
    if (e == hipSuccess) {
        *c->dem_host = 0;
        e = hipHostGetDevicePointer((void**)&c->dem_host_dev, c->dem_host, 0);
    }
    if (e != hipSuccess) {
        nfcs_ctx_destroy(c);
        return hip_fail(e);
    }
    *out = c;
    return NFCS_OK;
}

NFCS_API int nfcs_ctx_destroy(nfcs_ctx* c) {
    if (!c) return NFCS_OK;
    DeviceGuard dg_(c->di.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ws_used && !c->ws_own && c->ws_ev) (void)hipEventSynchronize(c->ws_ev);  // a caller stream's last write pass
    if (c->eq_used && !c->eq_own && c->eq_ev) (void)hipEventSynchronize(c->eq_ev);  // a caller stream's last enqueue
    if (c->ct_used && !c->ct_own && c->ct_ev) (void)hipEventSynchronize(c->ct_ev);  // a caller stream's last fold
    free_host_pipeline(c);
    if (c->d_digest) (void)hipFree(c->d_digest);
    if (c->eq_ws) (void)hipFree(c->eq_ws);
    if (c->eq_ev) (void)hipEventDestroy(c->eq_ev);
    if (c->ct_ws) (void)hipFree(c->ct_ws);
    if (c->ct_ev) (void)hipEventDestroy(c->ct_ev);
    if (c->ws) (void)hipFree(c->ws);
    if (c->ws_ev) (void)hipEventDestroy(c->ws_ev);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->obs_host) (void)hipHostFree(c->obs_host);
    if (c->dem_host) (void)hipHostFree(c->dem_host);
    if (c->dem_dev) (void)hipFree(c->dem_dev);
    delete c;
    return NFCS_OK;
}

NFCS_API void* nfcs_ctx_stream(nfcs_ctx* c) { return c ? (void*)c->stream : nullptr; }

NFCS_API int nfcs_ctx_set_slot_bytes(nfcs_ctx* c, uint32_t bytes) {
    if (!c) return NFCS_EINVAL;
    c->slot_bytes = bytes;
    return NFCS_OK;
}

NFCS_API int nfcs_ctx_set_store_policy(nfcs_ctx* c, int policy) {
    if (!c || (policy != NFCS_STORE_AUTO && policy != NFCS_STORE_DEFERRED && policy != NFCS_STORE_SPARSE))
        return NFCS_EINVAL;
    c->store_policy = policy;
    return NFCS_OK;
}

NFCS_API int nfcs_ctx_store_state(nfcs_ctx* c, int* form, uint32_t* sampled, uint32_t* storing) {
    if (!c) return NFCS_EINVAL;
    read_store_demand(c);
    if (form) *form = c->dem_last_form;
    if (sampled) *sampled = c->dem_policy.obs_sampled;
    if (storing) *storing = c->dem_policy.obs_storing;
    return NFCS_OK;
}

NFCS_API int nfcs_ctx_launch_footprint(nfcs_ctx* c, uint64_t arena_bytes, const nfcs_desc* d_desc,
                                       uint32_t n, uint64_t* mean) {
    if (!c || !mean) return NFCS_EINVAL;
    int slot = -1;
    *mean = peek_shape(c, arena_bytes, d_desc, n, &slot).mean;
    return NFCS_OK;
}

NFCS_API int nfcs_ctx_host_numa(nfcs_ctx* c, int* node, int* local) {
    if (!c || !node || !local) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the pipeline is built on the context's device
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    const int rc = ensure_host_pipeline(c);
    if (rc) return rc;
    *node = c->numa_node;
    *local = c->numa_local ? 1 : 0;
    return NFCS_OK;
}

NFCS_API int nfcs_update_device(nfcs_ctx* c, uint8_t* d_arena, uint64_t arena_bytes,
                                const nfcs_desc* d_desc, uint32_t n, uint8_t* d_status,
                                nfcs_patch* d_patch, void* stream) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    return update_device(c, d_arena, arena_bytes, d_desc, n, d_status, d_patch, pick(c, stream));
}

NFCS_API int nfcs_l3_forward_device(nfcs_ctx* c, uint8_t* d_arena, uint64_t arena_bytes,
                                    const nfcs_desc* d_desc, const uint32_t* d_nh, uint32_t n,
                                    const nfcs_nexthop* d_table, uint32_t table_n,
                                    uint8_t* d_status, void* stream) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || !d_nh || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    if (table_n > 0 && (!d_table || ((uintptr_t)d_table & 3u))) return NFCS_EINVAL;
    return l3_forward_device(c, d_arena, arena_bytes, d_desc, d_nh, n, d_table, table_n, d_status,
                             pick(c, stream));
}

NFCS_API int nfcs_vlan_device(nfcs_ctx* c, uint8_t* d_arena, uint64_t arena_bytes,
                              nfcs_desc* d_desc, uint32_t n, const uint32_t* d_ops,
                              uint32_t op_all, const uint32_t* d_caps, uint32_t cap_all,
                              uint8_t* d_status, void* stream) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    if (((uintptr_t)d_ops & 3u) || ((uintptr_t)d_caps & 3u)) return NFCS_EINVAL;
    const Shape sh = launch_shape(c, arena_bytes, d_desc, n, kVlanRule);
    NFCS_HIP(nfcs::launch_vlan(c->di, d_arena, arena_bytes, d_desc, n, d_ops, op_all, d_caps,
                               cap_all, d_status, pick(c, stream), sh.mean, sh.obs, sh.bits));
    return NFCS_OK;
}

NFCS_API int nfcs_flow_keys_device(nfcs_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes,
                                   const nfcs_desc* d_desc, uint32_t n, nfcs_flow_key* d_keys,
                                   uint32_t* d_hash, void* stream) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || ((uintptr_t)d_arena & 15u) || ((uintptr_t)d_keys & 15u))
        return NFCS_EINVAL;
    NFCS_HIP(nfcs::launch_flow_keys(c->di, d_arena, arena_bytes, d_desc, n, d_keys, d_hash,
                                    pick(c, stream)));
    return NFCS_OK;
}

// ---- forwarding table (nfcs_fib.h: inputs, commit, host decision) and its lookup kernel ----------
}  // extern "C"

struct nfcs_fib : Table<nfcs::FibInputs, nfcs::FibTables, nfcs::FibDev> {
    const nfcs_nexthop* d_table = nullptr;
    uint32_t d_table_n = 0;  // the table as uploaded (a later commit does not change it)
    void drop_upload() {
        Table::drop_upload();
        d_table = nullptr;
        d_table_n = 0;
    }
};

extern "C" {

NFCS_API int nfcs_fib_create(nfcs_fib** out) { return table_create(out); }
NFCS_API int nfcs_fib_destroy(nfcs_fib* f) { return table_destroy(f); }

NFCS_API int nfcs_fib_set_routes(nfcs_fib* f, const nfcs_fib_route* routes, uint32_t n) {
    if (n > NFCS_FIB_MAX_ROUTES) return NFCS_EINVAL;
    return table_assign(f, &nfcs::FibInputs::routes, routes, n);
}
NFCS_API int nfcs_fib_set_arp(nfcs_fib* f, const nfcs_fib_arp* arp, uint32_t n) {
    return table_assign(f, &nfcs::FibInputs::arp, arp, n);
}
NFCS_API int nfcs_fib_set_if_macs(nfcs_fib* f, const nfcs_fib_if_mac* if_macs, uint32_t n) {
    return table_assign(f, &nfcs::FibInputs::if_macs, if_macs, n);
}
NFCS_API int nfcs_fib_set_local_ips(nfcs_fib* f, const uint32_t* ips, uint32_t n) {
    return table_assign(f, &nfcs::FibInputs::local_ips, ips, n);
}

NFCS_API int nfcs_fib_commit(nfcs_fib* f) { return table_commit(f, nfcs::fib_compile); }

NFCS_API int nfcs_fib_upload(nfcs_ctx* c, nfcs_fib* f) {
    if (!c || !f || !f->committed) return NFCS_EINVAL;
    const nfcs::FibTables& t = f->t;
    BlobLayout lay;
    const size_t o_nm = lay.part(t.rt_nm), o_info = lay.part(t.rt_info), o_aip = lay.part(t.arp_ip);
    const size_t o_anh = lay.part(t.arp_nh), o_loc = lay.part(t.local_ip), o_tab = lay.part(t.table);
    return table_upload(c, f, lay, [&](const uint8_t* d) {
        f->dev.rt_nm = (const uint2*)(d + o_nm);
        f->dev.rt_info = (const uint2*)(d + o_info);
        f->dev.routes = t.routes;
        f->dev.routes_padded = (uint32_t)t.rt_nm.size();
        f->dev.arp_ip = (const uint32_t*)(d + o_aip);
        f->dev.arp_nh = (const uint32_t*)(d + o_anh);
        f->dev.arps = (uint32_t)t.arp_ip.size();
        f->dev.local_ip = (const uint32_t*)(d + o_loc);
        f->dev.locals = (uint32_t)t.local_ip.size();
        f->d_table = t.table.empty() ? nullptr : (const nfcs_nexthop*)(d + o_tab);
        f->d_table_n = (uint32_t)t.table.size();
    });
}

NFCS_API int nfcs_fib_nexthops(const nfcs_fib* f, const nfcs_nexthop** d_table, uint32_t* table_n) {
    if (!f || !f->uploaded || !d_table || !table_n) return NFCS_EINVAL;
    *d_table = f->d_table;
    *table_n = f->d_table_n;
    return NFCS_OK;
}

NFCS_API int nfcs_fib_nexthops_host(const nfcs_fib* f, nfcs_nexthop* out, uint32_t cap, uint32_t* table_n) {
    if (!f || !f->committed || !table_n) return NFCS_EINVAL;
    const uint32_t tn = (uint32_t)f->t.table.size();
    if (out && cap && tn) memcpy(out, f->t.table.data(), sizeof(nfcs_nexthop) * (cap < tn ? cap : tn));
    *table_n = tn;
    return NFCS_OK;
}

NFCS_API int nfcs_fib_lookup_host(const nfcs_fib* f, uint32_t dst_ip, uint32_t ttl, uint32_t* verdict,
                                  uint32_t* nh, uint32_t* egress_if) {
    if (!f || !f->committed) return NFCS_EINVAL;
    nfcs::fib_decide(f->t, dst_ip, ttl, verdict, nh, egress_if);
    return NFCS_OK;
}

NFCS_API int nfcs_route_lookup_device(nfcs_ctx* c, const nfcs_fib* f, const uint8_t* d_arena,
                                      uint64_t arena_bytes, const nfcs_desc* d_desc, uint32_t n,
                                      uint32_t* d_nh, uint32_t* d_egress_if, uint8_t* d_verdict,
                                      void* stream) {
    if (!usable(c, f)) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || !d_nh || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    if (((uintptr_t)d_nh & 3u) || ((uintptr_t)d_egress_if & 3u)) return NFCS_EINVAL;
    NFCS_HIP(nfcs::launch_route_lookup(c->di, f->dev, d_arena, arena_bytes, d_desc, n, d_nh, d_egress_if,
                                       d_verdict, pick(c, stream)));
    return NFCS_OK;
}

// ---- ACL (nfcs_acl.h: compile, host decision) and its evaluation kernel --------------------------
}  // extern "C"

struct nfcs_acl : Table<std::vector<nfcs_acl_rule>, nfcs::AclTables, nfcs::AclDev> {};

extern "C" {

NFCS_API int nfcs_acl_create(nfcs_acl** out) { return table_create(out); }
NFCS_API int nfcs_acl_destroy(nfcs_acl* a) { return table_destroy(a); }

NFCS_API int nfcs_acl_set_rules(nfcs_acl* a, const nfcs_acl_rule* rules, uint32_t n) {
    if (!a || (n > 0 && !rules) || n > NFCS_ACL_MAX_RULES) return NFCS_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if ((rules[i].fields & ~NFCS_ACL_F_ALL) || rules[i].action > NFCS_ACL_REDIRECT) return NFCS_EINVAL;
    return table_set(a, [&] { a->in.assign(rules, rules + n); });
}

NFCS_API int nfcs_acl_commit(nfcs_acl* a) { return table_commit(a, nfcs::acl_compile); }

NFCS_API int nfcs_acl_upload(nfcs_ctx* c, nfcs_acl* a) {
    if (!c || !a || !a->committed) return NFCS_EINVAL;
    const nfcs::AclTables& t = a->t;
    BlobLayout lay;
    const size_t o_rec = lay.part(t.rec), o_act = lay.part(t.act);  // the records are 64 bytes each
    return table_upload(c, a, lay, [&](const uint8_t* d) {
        a->dev.rec = (const uint4*)(d + o_rec);
        a->dev.act = (const uint2*)(d + o_act);
        a->dev.rules = t.rules;
        a->dev.rules_padded = (uint32_t)t.rec.size();
    });
}

NFCS_API int nfcs_acl_eval_host(const nfcs_acl* a, const uint8_t* frame, uint32_t len, uint32_t* action,
                                uint32_t* rule_index, uint32_t* redirect_port) {
    if (!a || !a->committed || (len > 0 && !frame)) return NFCS_EINVAL;
    nfcs::acl_decide(a->t, frame, len, action, rule_index, redirect_port);
    return NFCS_OK;
}

NFCS_API int nfcs_acl_eval_device(nfcs_ctx* c, const nfcs_acl* a, const uint8_t* d_arena, uint64_t arena_bytes,
                                  const nfcs_desc* d_desc, uint32_t n, uint8_t* d_action, uint32_t* d_rule,
                                  uint32_t* d_redirect, uint32_t* d_nh, void* stream) {
    if (!usable(c, a)) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || !d_action || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    if (((uintptr_t)d_rule & 3u) || ((uintptr_t)d_redirect & 3u) || ((uintptr_t)d_nh & 3u)) return NFCS_EINVAL;
    NFCS_HIP(nfcs::launch_acl_eval(c->di, a->dev, d_arena, arena_bytes, d_desc, n, d_action, d_rule, d_redirect, d_nh,
                                   pick(c, stream)));
    return NFCS_OK;
}

// ---- L2 forwarding database (nfcs_fdb.h: compile, host decision) and its lookup kernel -----------
}  // extern "C"

struct nfcs_fdb : Table<nfcs::FdbInputs, nfcs::FdbTables, nfcs::FdbDev> {};

extern "C" {

NFCS_API int nfcs_fdb_create(nfcs_fdb** out) { return table_create(out); }
NFCS_API int nfcs_fdb_destroy(nfcs_fdb* f) { return table_destroy(f); }

NFCS_API int nfcs_fdb_set_entries(nfcs_fdb* f, const nfcs_fdb_entry* entries, uint32_t n) {
    if (n > NFCS_FDB_MAX_ENTRIES) return NFCS_EINVAL;
    return table_assign(f, &nfcs::FdbInputs::entries, entries, n);
}

NFCS_API int nfcs_fdb_set_port(nfcs_fdb* f, const nfcs_l2_port* port, const uint16_t* allowed_vlans,
                               uint32_t n_allowed) {
    if (!f || !port || (n_allowed > 0 && !allowed_vlans)) return NFCS_EINVAL;
    if (port->port_id >= NFCS_L2_MAX_PORTS || port->native_vlan > 4095u || port->type > 2u) return NFCS_EINVAL;
    for (uint32_t i = 0; i < n_allowed; ++i)
        if (allowed_vlans[i] > 4095u) return NFCS_EINVAL;
    return table_set(f, [&] {
        if (f->in.ports.size() <= port->port_id) f->in.ports.resize(port->port_id + 1u);
        nfcs::FdbPortIn& pi = f->in.ports[port->port_id];
        pi.allowed.assign(allowed_vlans, allowed_vlans + n_allowed);
        pi.port = *port;
        pi.set = true;
    });
}

NFCS_API int nfcs_fdb_clear_ports(nfcs_fdb* f) {
    return table_set(f, [&] { f->in.ports.clear(); });
}

NFCS_API int nfcs_fdb_commit(nfcs_fdb* f) { return table_commit(f, nfcs::fdb_compile); }

NFCS_API int nfcs_fdb_upload(nfcs_ctx* c, nfcs_fdb* f) {
    if (!c || !f || !f->committed) return NFCS_EINVAL;
    const nfcs::FdbTables& t = f->t;
    BlobLayout lay;  // the slots (up to tens of MiB) are copied from where they are, like every part
    const size_t o_slots = lay.part(t.slots), o_vlans = lay.part(t.port_vlans), o_native = lay.part(t.port_native);
    const size_t o_state = lay.part(t.port_state), o_rows = lay.part(t.vlan_ports);
    return table_upload(c, f, lay, [&](const uint8_t* d) {
        f->dev.slots = (const uint4*)(d + o_slots);
        f->dev.slot_mask = (uint32_t)t.slots.size() - 1u;
        f->dev.max_probe = t.max_probe;
        f->dev.port_vlans = (const uint32_t*)(d + o_vlans);
        f->dev.port_native = (const uint16_t*)(d + o_native);
        f->dev.port_state = d + o_state;
        f->dev.ports = t.ports;
        f->dev.vlan_ports = (const uint32_t*)(d + o_rows);
        f->dev.port_words = t.port_words;
    });
}

NFCS_API int nfcs_fdb_stats(const nfcs_fdb* f, uint32_t* entries, uint32_t* slots, uint32_t* max_probe,
                            uint32_t* wrapped) {
    if (!f || !f->committed) return NFCS_EINVAL;
    if (entries) *entries = f->t.entries;
    if (slots) *slots = (uint32_t)f->t.slots.size();
    if (max_probe) *max_probe = f->t.max_probe;
    if (wrapped) *wrapped = f->t.wrapped;
    return NFCS_OK;
}

NFCS_API int nfcs_fdb_lookup_host(const nfcs_fdb* f, uint32_t ingress_port, const uint8_t* frame, uint32_t len,
                                  uint32_t* verdict, uint32_t* egress_port, uint32_t* vlan, uint32_t* learn) {
    if (!f || !f->committed || (len > 0 && !frame)) return NFCS_EINVAL;
    nfcs::fdb_decide(f->t, ingress_port, frame, len, verdict, egress_port, vlan, learn);
    return NFCS_OK;
}

NFCS_API int nfcs_fdb_flood_ports_host(const nfcs_fdb* f, uint32_t ingress_port, uint32_t vlan, uint32_t num_ports,
                                       uint32_t* ports, uint32_t cap, uint32_t* n) {
    if (!f || !f->committed || !n || (cap > 0 && !ports)) return NFCS_EINVAL;
    *n = nfcs::fdb_flood_ports(f->t, ingress_port, vlan, num_ports, ports, cap);
    return NFCS_OK;
}

NFCS_API int nfcs_l2_lookup_device(nfcs_ctx* c, const nfcs_fdb* f, uint32_t ingress_port, const uint8_t* d_arena,
                                   uint64_t arena_bytes, const nfcs_desc* d_desc, uint32_t n,
                                   const uint8_t* d_rt_verdict, uint32_t* d_egress_port, uint8_t* d_verdict,
                                   uint16_t* d_vlan, uint8_t* d_learn, void* stream) {
    if (!usable(c, f)) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || !d_egress_port || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    if (((uintptr_t)d_egress_port & 3u) || ((uintptr_t)d_vlan & 1u)) return NFCS_EINVAL;
    NFCS_HIP(nfcs::launch_l2_lookup(c->di, f->dev, ingress_port, d_arena, arena_bytes, d_desc, n, d_rt_verdict,
                                    d_egress_port, d_verdict, d_vlan, d_learn, pick(c, stream)));
    return NFCS_OK;
}

// ---- Flood replication (nfcs_fdb.h: the flood mask and the host walk) and its kernels ---------------

NFCS_API int nfcs_flood_expand_host(const nfcs_fdb* f, uint32_t ingress_port, uint32_t num_ports, uint64_t arena_bytes,
                                    uint64_t copy_base, uint32_t copy_align, const nfcs_desc* desc, uint32_t n,
                                    const uint32_t* l3_port, const uint8_t* fwd_status, const uint32_t* l2_port,
                                    const uint8_t* l2_verdict, const uint16_t* l2_vlan, uint32_t cap,
                                    nfcs_desc* item_desc, uint32_t* item_port, uint32_t* item_src,
                                    nfcs_flood_totals* totals) {
    if (!f || !f->committed) return NFCS_EINVAL;
    if (!nfcs::flood_args_ok(num_ports, arena_bytes, copy_base, copy_align, n, l3_port, fwd_status, l2_port, l2_verdict,
                             l2_vlan))
        return NFCS_EINVAL;
    if (n == 0) return NFCS_OK;
    if (!desc || !totals || (cap > 0 && (!item_desc || !item_port || !item_src))) return NFCS_EINVAL;
    nfcs::flood_expand(f->t, ingress_port, num_ports, arena_bytes, copy_base, copy_align, desc, n, l3_port, fwd_status,
                       l2_port, l2_verdict, l2_vlan, cap, item_desc, item_port, item_src, totals);
    return NFCS_OK;
}

NFCS_API int nfcs_flood_expand_device(nfcs_ctx* c, const nfcs_fdb* f, uint32_t ingress_port, uint32_t num_ports,
                                      uint8_t* d_arena, uint64_t arena_bytes, uint64_t copy_base, uint32_t copy_align,
                                      const nfcs_desc* d_desc, uint32_t n, const uint32_t* d_l3_port,
                                      const uint8_t* d_fwd_status, const uint32_t* d_l2_port,
                                      const uint8_t* d_l2_verdict, const uint16_t* d_l2_vlan, uint32_t cap,
                                      nfcs_desc* d_item_desc, uint32_t* d_item_port, uint32_t* d_item_src,
                                      nfcs_flood_totals* d_totals, void* stream) {
    if (!usable(c, f)) return NFCS_EINVAL;
    if (!nfcs::flood_args_ok(num_ports, arena_bytes, copy_base, copy_align, n, d_l3_port, d_fwd_status, d_l2_port,
                             d_l2_verdict, d_l2_vlan))
        return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || !d_totals || ((uintptr_t)d_arena & 15u) || ((uintptr_t)d_totals & 7u)) return NFCS_EINVAL;
    if (cap > 0 && (!d_item_desc || !d_item_port || !d_item_src)) return NFCS_EINVAL;
    if (((uintptr_t)d_l3_port & 3u) || ((uintptr_t)d_l2_port & 3u) || ((uintptr_t)d_l2_vlan & 1u) ||
        ((uintptr_t)d_item_desc & 7u) || ((uintptr_t)d_item_port & 3u) || ((uintptr_t)d_item_src & 3u))
        return NFCS_EINVAL;
    hipStream_t st = pick(c, stream);
    const nfcs::FloodArgs a{d_arena, arena_bytes, copy_base, copy_align, ingress_port, num_ports, n, cap, d_desc,
                            d_l3_port, d_fwd_status, d_l2_port, d_l2_verdict, d_l2_vlan, d_item_desc, d_item_port,
                            d_item_src, d_totals};
    return with_eq_scratch(c, nfcs::flood_scratch_words(n), st, [&](uint32_t* ws) {
        return nfcs::launch_flood_expand(c->di, f->dev, a, ws, st);
    });
}

// ---- ICMP responder (nfcs_icmp.h: compile, the plan, the host walk) and its kernels -----------------
}  // extern "C"

struct nfcs_icmp : Table<nfcs::IcmpInputs, nfcs::IcmpTables, nfcs::IcmpView> {};

namespace {
nfcs::FibView fib_dev_view(const nfcs_fib* f) {
    return nfcs::FibView{(const nfcs::U2*)f->dev.rt_nm, (const nfcs::U2*)f->dev.rt_info, f->dev.routes_padded,
                         f->dev.arp_ip, f->dev.arp_nh, f->dev.arps, f->d_table};
}
}  // namespace

extern "C" {

NFCS_API int nfcs_icmp_create(nfcs_icmp** out) { return table_create(out); }
NFCS_API int nfcs_icmp_destroy(nfcs_icmp* m) { return table_destroy(m); }

NFCS_API int nfcs_icmp_set_local(nfcs_icmp* m, const nfcs_icmp_local* local, uint32_t n) {
    return table_assign(m, &nfcs::IcmpInputs::local, local, n);
}
NFCS_API int nfcs_icmp_set_if_ips(nfcs_icmp* m, const nfcs_icmp_if_ip* if_ips, uint32_t n) {
    return table_assign(m, &nfcs::IcmpInputs::if_ips, if_ips, n);
}
NFCS_API int nfcs_icmp_set_ports_up(nfcs_icmp* m, const uint32_t* ports, uint32_t n, uint32_t num_ports) {
    if (!m || num_ports > nfcs::kIcmpMaxPorts) return NFCS_EINVAL;
    const int rc = table_assign(m, &nfcs::IcmpInputs::up, ports, n);
    if (rc == NFCS_OK) m->in.num_ports = num_ports;
    return rc;
}

NFCS_API int nfcs_icmp_commit(nfcs_icmp* m) { return table_commit(m, nfcs::icmp_compile); }

NFCS_API int nfcs_icmp_upload(nfcs_ctx* c, nfcs_icmp* m) {
    if (!c || !m || !m->committed) return NFCS_EINVAL;
    const nfcs::IcmpTables& t = m->t;
    BlobLayout lay;
    const size_t o_lip = lay.part(t.local_ip), o_lmac = lay.part(t.local_mac), o_iid = lay.part(t.if_id);
    const size_t o_iip = lay.part(t.if_ip), o_up = lay.part(t.up);
    return table_upload(c, m, lay, [&](const uint8_t* d) {
        m->dev = nfcs::IcmpView{(const uint32_t*)(d + o_lip), (const nfcs::U2*)(d + o_lmac), (uint32_t)t.local_ip.size(),
                                (const uint32_t*)(d + o_iid), (const uint32_t*)(d + o_iip), (uint32_t)t.if_id.size(),
                                (const uint32_t*)(d + o_up), t.num_ports};
    });
}

NFCS_API int nfcs_fib_resolve_host(const nfcs_fib* f, uint32_t ip, uint32_t* verdict, uint32_t* nh, uint32_t* egress_if) {
    if (!f || !f->committed) return NFCS_EINVAL;
    uint32_t v, h, e;
    nfcs::fib_resolve(nfcs::fib_view(f->t), ip, &v, &h, &e);
    if (verdict) *verdict = v;
    if (nh) *nh = h;
    if (egress_if) *egress_if = e;
    return NFCS_OK;
}

NFCS_API int nfcs_icmp_respond_host(const nfcs_icmp* m, const nfcs_fib* f, uint32_t ingress_port, uint8_t* arena,
                                    uint64_t arena_bytes, uint64_t msg_base, uint32_t msg_align, const nfcs_desc* desc,
                                    uint32_t n, const uint8_t* rt_verdict, const uint16_t* ip_id, uint32_t cap,
                                    nfcs_desc* msg_desc, uint32_t* msg_port, uint32_t* msg_src, uint8_t* status,
                                    nfcs_icmp_totals* totals) {
    if (!m || !m->committed || !f || !f->committed) return NFCS_EINVAL;
    if (!nfcs::icmp_args_ok(arena_bytes, msg_base, msg_align)) return NFCS_EINVAL;
    if (n == 0) return NFCS_OK;
    if (!arena || !desc || !rt_verdict || !totals || (cap > 0 && (!msg_desc || !msg_port || !msg_src))) return NFCS_EINVAL;
    try {
        nfcs::icmp_respond(m->t, f->t, ingress_port, arena, arena_bytes, msg_base, msg_align, desc, n, rt_verdict, ip_id,
                           cap, msg_desc, msg_port, msg_src, status, totals);
    } catch (...) {
        return NFCS_ENOMEM;
    }
    return NFCS_OK;
}

NFCS_API int nfcs_icmp_respond_device(nfcs_ctx* c, const nfcs_icmp* m, const nfcs_fib* f, uint32_t ingress_port,
                                      uint8_t* d_arena, uint64_t arena_bytes, uint64_t msg_base, uint32_t msg_align,
                                      const nfcs_desc* d_desc, uint32_t n, const uint8_t* d_rt_verdict,
                                      const uint16_t* d_ip_id, uint32_t cap, nfcs_desc* d_msg_desc, uint32_t* d_msg_port,
                                      uint32_t* d_msg_src, uint8_t* d_status, nfcs_icmp_totals* d_totals, void* stream) {
    if (!usable(c, m)) return NFCS_EINVAL;
    if (!usable(c, f)) return NFCS_EINVAL;
    if (!nfcs::icmp_args_ok(arena_bytes, msg_base, msg_align)) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || !d_rt_verdict || !d_totals || ((uintptr_t)d_arena & 15u) || ((uintptr_t)d_totals & 7u))
        return NFCS_EINVAL;
    if (cap > 0 && (!d_msg_desc || !d_msg_port || !d_msg_src)) return NFCS_EINVAL;
    if (((uintptr_t)d_ip_id & 1u) || ((uintptr_t)d_msg_desc & 7u) || ((uintptr_t)d_msg_port & 3u) ||
        ((uintptr_t)d_msg_src & 3u))
        return NFCS_EINVAL;
    hipStream_t st = pick(c, stream);
    const nfcs::IcmpArgs a{d_arena, arena_bytes, msg_base, msg_align, ingress_port, n, cap, d_desc, d_rt_verdict, d_ip_id,
                           d_msg_desc, d_msg_port, d_msg_src, d_status, d_totals};
    return with_eq_scratch(c, nfcs::flood_scratch_words(n), st, [&](uint32_t* ws) {
        return nfcs::launch_icmp_respond(c->di, m->dev, fib_dev_view(f), a, ws, st);
    });
}

// ---- Egress stage (nfcs_egress.h: compile, host plan, host enqueue) and its kernels ----------------
}  // extern "C"

struct nfcs_egress : Table<nfcs::EgressInputs, nfcs::EgressTables, nfcs::EgressDev> {};

extern "C" {

NFCS_API int nfcs_egress_create(nfcs_egress** out) { return table_create(out); }
NFCS_API int nfcs_egress_destroy(nfcs_egress* g) { return table_destroy(g); }

NFCS_API int nfcs_egress_set_port(nfcs_egress* g, const nfcs_egress_port* port) {
    if (!g || !port) return NFCS_EINVAL;
    if (port->port_id >= NFCS_L2_MAX_PORTS || port->type > 2u || port->native_vlan > 4095u ||
        port->num_queues > NFCS_QOS_MAX_QUEUES)
        return NFCS_EINVAL;
    return table_set(g, [&] {
        if (g->in.ports.size() <= port->port_id) g->in.ports.resize(port->port_id + 1u);
        g->in.ports[port->port_id].port = *port;
        g->in.ports[port->port_id].set = true;
    });
}

NFCS_API int nfcs_egress_clear_ports(nfcs_egress* g) {
    return table_set(g, [&] { g->in.ports.clear(); });
}

NFCS_API int nfcs_egress_commit(nfcs_egress* g) { return table_commit(g, nfcs::egress_compile); }

NFCS_API int nfcs_egress_upload(nfcs_ctx* c, nfcs_egress* g) {
    if (!c || !g || !g->committed) return NFCS_EINVAL;
    BlobLayout lay;
    const size_t o_recs = lay.part(g->t.recs);
    return table_upload(c, g, lay, [&](const uint8_t* d) {
        g->dev.recs = (const uint4*)(d + o_recs);
        g->dev.ports = g->t.ports;
        g->dev.keys = g->t.keys;
    });
}

NFCS_API int nfcs_egress_keys(const nfcs_egress* g, uint32_t* ports, uint32_t* keys) {
    if (!g || !g->committed) return NFCS_EINVAL;
    if (ports) *ports = g->t.ports;
    if (keys) *keys = g->t.keys;
    return NFCS_OK;
}

NFCS_API int nfcs_egress_plan_host(const nfcs_egress* g, uint32_t port, const uint8_t* frame, uint32_t len,
                                   uint32_t* op, uint32_t* queue) {
    if (!g || !g->committed || (len > 0 && !frame)) return NFCS_EINVAL;
    nfcs::egress_plan(g->t, port, frame, len, op, queue);
    return NFCS_OK;
}

NFCS_API int nfcs_egress_enqueue_host(const nfcs_egress* g, const uint32_t* port, const uint8_t* queue, uint32_t n,
                                      uint32_t* depth, uint8_t* result, uint32_t* order, uint32_t* key_start,
                                      uint32_t* key_dropped) {
    if (!g || !g->committed || !key_start || (g->t.keys > 0 && !depth)) return NFCS_EINVAL;
    if (n > 0 && (!port || !queue || !order)) return NFCS_EINVAL;
    try {
        nfcs::egress_enqueue(g->t, port, queue, n, depth, result, order, key_start, key_dropped);
    } catch (...) {
        return NFCS_ENOMEM;
    }
    return NFCS_OK;
}

NFCS_API int nfcs_egress_plan_device(nfcs_ctx* c, const nfcs_egress* g, const uint8_t* d_arena, uint64_t arena_bytes,
                                     const nfcs_desc* d_desc, uint32_t n, const uint32_t* d_l3_port,
                                     const uint8_t* d_fwd_status, const uint32_t* d_l2_port, uint32_t* d_port,
                                     uint32_t* d_ops, uint8_t* d_queue, void* stream) {
    if (!usable(c, g)) return NFCS_EINVAL;
    if ((!d_l3_port && !d_l2_port) || (d_fwd_status && !d_l3_port)) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || !d_port || !d_ops || !d_queue || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    if (((uintptr_t)d_l3_port & 3u) || ((uintptr_t)d_l2_port & 3u) || ((uintptr_t)d_port & 3u) || ((uintptr_t)d_ops & 3u))
        return NFCS_EINVAL;
    NFCS_HIP(nfcs::launch_egress_plan(c->di, g->dev, d_arena, arena_bytes, d_desc, n, d_l3_port, d_fwd_status, d_l2_port,
                                      d_port, d_ops, d_queue, pick(c, stream)));
    return NFCS_OK;
}

NFCS_API int nfcs_egress_enqueue_device(nfcs_ctx* c, const nfcs_egress* g, const uint32_t* d_port, const uint8_t* d_queue,
                                        uint32_t n, uint32_t* d_depth, uint8_t* d_result, uint32_t* d_order,
                                        uint32_t* d_key_start, uint32_t* d_key_dropped, void* stream) {
    if (!usable(c, g)) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_port || !d_queue || !d_order || !d_key_start || (g->dev.keys > 0 && !d_depth)) return NFCS_EINVAL;
    if (((uintptr_t)d_port & 3u) || ((uintptr_t)d_depth & 3u) || ((uintptr_t)d_order & 3u) ||
        ((uintptr_t)d_key_start & 3u) || ((uintptr_t)d_key_dropped & 3u))
        return NFCS_EINVAL;
    hipStream_t st = pick(c, stream);
    return with_eq_scratch(c, nfcs::egress_scratch_words(n, g->dev.keys), st, [&](uint32_t* ws) {
        return nfcs::launch_egress_enqueue(c->di, g->dev, d_port, d_queue, n, d_depth, d_result, d_order, d_key_start,
                                           d_key_dropped, ws, st);
    });
}

// ---- Egress ACLs (nfcs_aclset.h: lists, bindings, compile, host decision) and their kernel ---------
}  // extern "C"

struct nfcs_aclset : Table<nfcs::AclSetInputs, nfcs::AclSetTables, nfcs::AclSetDev> {};

extern "C" {

NFCS_API int nfcs_aclset_create(nfcs_aclset** out) { return table_create(out); }
NFCS_API int nfcs_aclset_destroy(nfcs_aclset* s) { return table_destroy(s); }

NFCS_API int nfcs_aclset_set_list(nfcs_aclset* s, uint32_t list_id, const nfcs_acl_rule* rules, uint32_t n) {
    return table_set(s, [&] { return nfcs::aclset_set_list(s->in, list_id, rules, n); });
}
NFCS_API int nfcs_aclset_remove_list(nfcs_aclset* s, uint32_t list_id) {
    return table_set(s, [&] { return nfcs::aclset_remove_list(s->in, list_id); });
}
NFCS_API int nfcs_aclset_bind_port(nfcs_aclset* s, uint32_t port_id, uint32_t list_id) {
    return table_set(s, [&] { return nfcs::aclset_bind_port(s->in, port_id, list_id); });
}
NFCS_API int nfcs_aclset_clear(nfcs_aclset* s) {
    return table_set(s, [&] { nfcs::aclset_clear(s->in); });
}

NFCS_API int nfcs_aclset_commit(nfcs_aclset* s) { return table_commit(s, nfcs::aclset_compile); }

NFCS_API int nfcs_aclset_upload(nfcs_ctx* c, nfcs_aclset* s) {
    if (!c || !s || !s->committed) return NFCS_EINVAL;
    const nfcs::AclSetTables& t = s->t;
    BlobLayout lay;  // the records (64 bytes each), the actions, the ports' bindings (8 bytes each)
    const size_t o_rec = lay.part(t.rec), o_act = lay.part(t.act), o_bind = lay.part(t.bind);
    return table_upload(c, s, lay, [&](const uint8_t* d) {
        s->dev.rec = (const uint4*)(d + o_rec);
        s->dev.act = (const uint2*)(d + o_act);
        s->dev.bind = (const uint2*)(d + o_bind);
        s->dev.ports = t.ports;
        s->dev.rules_padded = (uint32_t)t.rec.size();
    });
}

NFCS_API int nfcs_aclset_info(const nfcs_aclset* s, uint32_t* ports, uint32_t* lists, uint32_t* rules_padded) {
    if (!s || !s->committed) return NFCS_EINVAL;
    if (ports) *ports = s->t.ports;
    if (lists) *lists = s->t.lists;
    if (rules_padded) *rules_padded = (uint32_t)s->t.rec.size();
    return NFCS_OK;
}

NFCS_API int nfcs_aclset_eval_host(const nfcs_aclset* s, uint32_t port, const uint8_t* frame, uint32_t len,
                                   uint32_t* action, uint32_t* rule_index, uint32_t* redirect_port) {
    if (!s || !s->committed || (len > 0 && !frame)) return NFCS_EINVAL;
    nfcs::aclset_decide(s->t, port, frame, len, action, rule_index, redirect_port);
    return NFCS_OK;
}

NFCS_API int nfcs_egress_acl_host(const nfcs_aclset* s, const uint8_t* arena, uint64_t arena_bytes,
                                  const nfcs_desc* desc, uint32_t n, uint32_t* port, uint8_t* action, uint32_t* rule,
                                  uint32_t* redirect, uint32_t* denied_pkts, uint64_t* denied_bytes) {
    if (!s || !s->committed || (!denied_pkts != !denied_bytes)) return NFCS_EINVAL;
    if (n == 0) return NFCS_OK;
    if (!arena || !desc || !port || !action) return NFCS_EINVAL;
    nfcs::aclset_egress(s->t, arena, arena_bytes, desc, n, port, action, rule, redirect, denied_pkts, denied_bytes);
    return NFCS_OK;
}

NFCS_API int nfcs_egress_acl_device(nfcs_ctx* c, const nfcs_aclset* s, const uint8_t* d_arena, uint64_t arena_bytes,
                                    const nfcs_desc* d_desc, uint32_t n, uint32_t* d_port, uint8_t* d_action,
                                    uint32_t* d_rule, uint32_t* d_redirect, uint32_t* d_denied_pkts,
                                    uint64_t* d_denied_bytes, void* stream) {
    if (!usable(c, s)) return NFCS_EINVAL;
    if (!d_denied_pkts != !d_denied_bytes) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || !d_port || !d_action || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    if (((uintptr_t)d_port & 3u) || ((uintptr_t)d_rule & 3u) || ((uintptr_t)d_redirect & 3u) ||
        ((uintptr_t)d_denied_pkts & 3u) || ((uintptr_t)d_denied_bytes & 7u))
        return NFCS_EINVAL;
    hipStream_t st = pick(c, stream);
    return with_ct_scratch(c, d_denied_pkts != nullptr, st, [&](uint64_t* ct) {
        return nfcs::launch_egress_acl(c->di, s->dev, d_arena, arena_bytes, d_desc, n, d_port, d_action, d_rule, d_redirect,
                                       d_denied_pkts, d_denied_bytes, ct, st);
    });
}

// ---- TX queues (nfcs_txq.h: tables, host state, the walks and the closed form) and their kernels ------
}  // extern "C"

struct nfcs_txq {
    nfcs::TxqTables t;
    nfcs::TxqState h;  // the host copy
    // the device copy (absent for a host-only object): tables, heads, last and scratch in d_blob, the rings
    // in d_ring
    nfcs_ctx* ctx = nullptr;
    int device = -1;
    uint8_t* d_blob = nullptr;
    uint8_t* d_ring = nullptr;
    size_t state_off = 0, state_bytes = 0;  // head and last within d_blob (what nfcs_txq_reset zeroes)
    nfcs::TxqDev dev;
};

namespace {
void txq_free_device(nfcs_txq* x) {
    if (x->d_blob || x->d_ring) {
        DeviceGuard dg_(x->device);
        if (dg_.err == hipSuccess) {
            if (x->d_blob) (void)hipFree(x->d_blob);
            if (x->d_ring) (void)hipFree(x->d_ring);
        }
    }
    x->d_blob = x->d_ring = nullptr;
    x->dev = nfcs::TxqDev{};
}

// Lays the device copy out in one allocation (every part 16-byte aligned) plus the rings, and uploads the
// tables; heads, last and scratch start as zero.
int txq_make_device(nfcs_ctx* c, nfcs_txq* x) {
    const nfcs::TxqTables& t = x->t;
    BlobLayout lay;
    const size_t o_port = lay.part(t.port);
    const size_t o_base = lay.part(t.ring_base);
    const size_t o_head = lay.part(nullptr, (size_t)t.keys * 4u);
    const size_t o_last = lay.part(nullptr, (size_t)t.ports * 4u);
    const size_t o_take = lay.part(nullptr, (size_t)t.keys * 4u);
    const size_t o_elem = lay.part(nullptr, ((size_t)t.keys + 1u) * 4u);
    const size_t o_txs = lay.part(nullptr, ((size_t)t.ports + 1u) * 4u);
    const size_t o_nl = lay.part(nullptr, (size_t)t.ports * 4u);
    if (t.ring_slots > (SIZE_MAX >> 4)) return NFCS_ENOMEM;
    DeviceGuard dg_(c->di.device);
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    x->device = c->di.device;
    hipError_t e = lay.upload(&x->d_blob);
    if (e == hipSuccess) e = hipMalloc(&x->d_ring, (size_t)t.ring_slots * 8u + 16u);
    if (e == hipSuccess) e = hipMemset(x->d_ring, 0, (size_t)t.ring_slots * 8u + 16u);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        txq_free_device(x);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return NFCS_ENOMEM;
        }
        return hip_fail(e);
    }
    x->state_off = o_head;
    x->state_bytes = o_take - o_head;  // head, then last
    nfcs::TxqDev& d = x->dev;
    d.port = (const uint4*)(x->d_blob + o_port);
    d.ring_base = (const uint64_t*)(x->d_blob + o_base);
    d.ring = (uint64_t*)x->d_ring;
    d.head = (uint32_t*)(x->d_blob + o_head);
    d.last = (uint32_t*)(x->d_blob + o_last);
    d.take = (uint32_t*)(x->d_blob + o_take);
    d.elem_start = (uint32_t*)(x->d_blob + o_elem);
    d.tx_start = (uint32_t*)(x->d_blob + o_txs);
    d.new_last = (uint32_t*)(x->d_blob + o_nl);
    d.ports = t.ports;
    d.keys = t.keys;
    d.ring_slots = t.ring_slots;
    x->ctx = c;
    return NFCS_OK;
}
}  // namespace

extern "C" {

NFCS_API int nfcs_txq_create(nfcs_ctx* c, const nfcs_egress* g, nfcs_txq** out) {
    if (!out) return NFCS_EINVAL;
    *out = nullptr;
    if (!g || !g->committed) return NFCS_EINVAL;
    nfcs_txq* x = new (std::nothrow) nfcs_txq();
    if (!x) return NFCS_ENOMEM;
    try {
        nfcs::txq_compile(g->t, x->t);
        nfcs::txq_state_init(x->t, x->h);
    } catch (...) {
        delete x;
        return NFCS_ENOMEM;
    }
    if (c) {
        const int rc = txq_make_device(c, x);
        if (rc != NFCS_OK) {
            delete x;
            return rc;
        }
    }
    *out = x;
    return NFCS_OK;
}

NFCS_API int nfcs_txq_destroy(nfcs_txq* x) {
    if (!x) return NFCS_EINVAL;
    txq_free_device(x);
    delete x;
    return NFCS_OK;
}

NFCS_API int nfcs_txq_set_scheduler(nfcs_txq* x, uint32_t port_id, uint32_t sched) {
    if (!x || port_id >= x->t.ports || sched > NFCS_SCHED_DRR) return NFCS_EINVAL;
    if (x->ctx) {
        DeviceGuard dg_(x->device);
        if (dg_.err != hipSuccess) return hip_fail(dg_.err);
        nfcs::TxqPort rec = x->t.port[port_id];
        rec.sched = sched;
        NFCS_HIP(hipMemcpy((uint8_t*)x->dev.port + (size_t)port_id * sizeof(rec), &rec, sizeof(rec), hipMemcpyHostToDevice));
        NFCS_HIP(hipDeviceSynchronize());
    }
    x->t.port[port_id].sched = sched;
    return NFCS_OK;
}

NFCS_API int nfcs_txq_reset(nfcs_txq* x) {
    if (!x) return NFCS_EINVAL;
    if (x->ctx) {
        DeviceGuard dg_(x->device);
        if (dg_.err != hipSuccess) return hip_fail(dg_.err);
        NFCS_HIP(hipDeviceSynchronize());  // the object must be idle; this makes it so
        if (x->state_bytes) NFCS_HIP(hipMemset(x->d_blob + x->state_off, 0, x->state_bytes));
        NFCS_HIP(hipDeviceSynchronize());
    }
    std::fill(x->h.head.begin(), x->h.head.end(), 0u);
    std::fill(x->h.last.begin(), x->h.last.end(), (uint8_t)0);
    return NFCS_OK;
}

NFCS_API int nfcs_txq_info(const nfcs_txq* x, uint32_t* ports, uint32_t* keys, uint64_t* ring_slots) {
    if (!x) return NFCS_EINVAL;
    if (ports) *ports = x->t.ports;
    if (keys) *keys = x->t.keys;
    if (ring_slots) *ring_slots = x->t.ring_slots;
    return NFCS_OK;
}

NFCS_API int nfcs_txq_state_host(const nfcs_txq* x, uint32_t* head, uint8_t* last) {
    if (!x) return NFCS_EINVAL;
    if (head && x->t.keys) memcpy(head, x->h.head.data(), (size_t)x->t.keys * 4u);
    if (last && x->t.ports) memcpy(last, x->h.last.data(), x->t.ports);
    return NFCS_OK;
}

NFCS_API int nfcs_txq_state_device(nfcs_txq* x, uint32_t* head, uint8_t* last, void* stream) {
    if (!x || !x->ctx) return NFCS_EINVAL;
    DeviceGuard dg_(x->device);
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    NFCS_HIP(hipStreamSynchronize(pick(x->ctx, stream)));
    if (head && x->t.keys) NFCS_HIP(hipMemcpy(head, x->dev.head, (size_t)x->t.keys * 4u, hipMemcpyDeviceToHost));
    if (last && x->t.ports) {
        std::vector<uint32_t> w;
        try {
            w.resize(x->t.ports);
        } catch (...) {
            return NFCS_ENOMEM;
        }
        NFCS_HIP(hipMemcpy(w.data(), x->dev.last, (size_t)x->t.ports * 4u, hipMemcpyDeviceToHost));
        for (uint32_t p = 0; p < x->t.ports; ++p) last[p] = (uint8_t)w[p];
    }
    return NFCS_OK;
}

NFCS_API int nfcs_txq_append_host(nfcs_txq* x, const uint32_t* order, const uint32_t* key_start, const uint32_t* depth,
                                  const uint64_t* handle, const nfcs_desc* desc, uint32_t n) {
    if (!x) return NFCS_EINVAL;
    if (n == 0) return NFCS_OK;
    if (!handle && !desc) return NFCS_EINVAL;
    if (!order || !key_start || (x->t.keys > 0 && !depth)) return NFCS_EINVAL;
    nfcs::txq_append(x->t, x->h, order, key_start, depth, handle, desc, n);
    return NFCS_OK;
}

NFCS_API int nfcs_txq_append_device(nfcs_ctx* c, nfcs_txq* x, const uint32_t* d_order, const uint32_t* d_key_start,
                                    const uint32_t* d_depth, const uint64_t* d_handle, const nfcs_desc* d_desc, uint32_t n,
                                    void* stream) {
    if (!c || !x || x->ctx != c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_handle && !d_desc) return NFCS_EINVAL;
    if (!d_order || !d_key_start || (x->dev.keys > 0 && !d_depth)) return NFCS_EINVAL;
    if (((uintptr_t)d_order & 3u) || ((uintptr_t)d_key_start & 3u) || ((uintptr_t)d_depth & 3u) ||
        ((uintptr_t)d_handle & 7u) || ((uintptr_t)d_desc & 7u))
        return NFCS_EINVAL;
    NFCS_HIP(nfcs::launch_txq_append(x->dev, d_order, d_key_start, d_depth, d_handle, d_desc, n, pick(c, stream)));
    return NFCS_OK;
}

NFCS_API int nfcs_txq_dequeue_host(nfcs_txq* x, const uint32_t* budget, uint32_t budget_all, uint32_t* depth, uint64_t* tx,
                                   uint32_t tx_cap, uint8_t* tx_queue, uint32_t* tx_start, uint32_t* dequeued) {
    if (!x || !tx_start || (x->t.keys > 0 && !depth) || (tx_cap > 0 && !tx)) return NFCS_EINVAL;
    nfcs::txq_dequeue_walk(x->t, x->h, budget, budget_all, depth, tx, tx_cap, tx_queue, tx_start, dequeued);
    return NFCS_OK;
}

NFCS_API int nfcs_txq_dequeue_device(nfcs_ctx* c, nfcs_txq* x, const uint32_t* d_budget, uint32_t budget_all,
                                     uint32_t* d_depth, uint64_t* d_tx, uint32_t tx_cap, uint8_t* d_tx_queue,
                                     uint32_t* d_tx_start, uint32_t* d_dequeued, void* stream) {
    if (!c || !x || x->ctx != c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (!d_tx_start || (x->dev.keys > 0 && !d_depth) || (tx_cap > 0 && !d_tx)) return NFCS_EINVAL;
    if (((uintptr_t)d_budget & 3u) || ((uintptr_t)d_depth & 3u) || ((uintptr_t)d_tx & 7u) || ((uintptr_t)d_tx_start & 3u) ||
        ((uintptr_t)d_dequeued & 3u))
        return NFCS_EINVAL;
    NFCS_HIP(nfcs::launch_txq_dequeue(x->dev, d_budget, budget_all, d_depth, d_tx, tx_cap, d_tx_queue, d_tx_start,
                                      d_dequeued, pick(c, stream)));
    return NFCS_OK;
}

NFCS_API int nfcs_txq_closed_form_host(uint32_t sched, uint32_t num_queues, uint32_t last, const uint32_t* depth,
                                       uint32_t budget, uint32_t* take, uint32_t* new_last, uint8_t* seq,
                                       uint32_t seq_cap) {
    if (sched > NFCS_SCHED_DRR || num_queues == 0 || num_queues > NFCS_QOS_MAX_QUEUES || last >= num_queues || !depth ||
        !take || !new_last)
        return NFCS_EINVAL;
    const nfcs::TxqPort pr{num_queues, 0xFFFFFFFFu, sched, 0u};
    uint32_t d8[nfcs::kTxqQ] = {0}, D[nfcs::kTxqQ], tk[nfcs::kTxqQ];
    for (uint32_t q = 0; q < num_queues; ++q) d8[q] = depth[q];
    const uint64_t sum = nfcs::txq_depths(pr, d8, D);
    const uint32_t G = (uint32_t)(sum < budget ? sum : budget);
    nfcs::txq_take(pr, last, D, G, tk, new_last);
    for (uint32_t q = 0; q < num_queues; ++q) {
        take[q] = tk[q];
        for (uint32_t r = 0; seq && r < tk[q]; ++r) {
            const uint64_t rank = nfcs::txq_rank(pr, last, D, q, r);
            if (rank < seq_cap) seq[rank] = (uint8_t)q;
        }
    }
    return NFCS_OK;
}

// ---- Ingress dispatch (nfcs_switch.h: the per-frame decision and the host walk) and the RX pipeline ------

NFCS_API int nfcs_ingress_dispatch_host(const nfcs_fdb* f, uint32_t ingress_port, uint32_t num_ports, const uint8_t* arena,
                                        uint64_t arena_bytes, const nfcs_desc* desc, uint32_t n, const uint8_t* action,
                                        const uint32_t* redirect, const uint8_t* rt_verdict, uint32_t* nh,
                                        uint32_t* l2_port, uint8_t* l2_verdict, uint8_t* cls, uint8_t* bypass,
                                        nfcs_rx_stats* rx_stats) {
    if (!f || !f->committed) return NFCS_EINVAL;
    if (n == 0) return NFCS_OK;
    if (!arena || !desc || !rt_verdict || !nh || !l2_port || !l2_verdict) return NFCS_EINVAL;
    nfcs::sw_dispatch(f->t.port_state.data(), f->t.ports, ingress_port, num_ports, arena, arena_bytes, desc, n, action,
                      redirect, rt_verdict, nh, l2_port, l2_verdict, cls, bypass, rx_stats);
    return NFCS_OK;
}

NFCS_API int nfcs_ingress_dispatch_device(nfcs_ctx* c, const nfcs_fdb* f, uint32_t ingress_port, uint32_t num_ports,
                                          const uint8_t* d_arena, uint64_t arena_bytes, const nfcs_desc* d_desc,
                                          uint32_t n, const uint8_t* d_action, const uint32_t* d_redirect,
                                          const uint8_t* d_rt_verdict, uint32_t* d_nh, uint32_t* d_l2_port,
                                          uint8_t* d_l2_verdict, uint8_t* d_class, uint8_t* d_bypass,
                                          nfcs_rx_stats* d_rx_stats, void* stream) {
    if (!usable(c, f)) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || !d_rt_verdict || !d_nh || !d_l2_port || !d_l2_verdict || ((uintptr_t)d_arena & 15u))
        return NFCS_EINVAL;
    if (((uintptr_t)d_redirect & 3u) || ((uintptr_t)d_nh & 3u) || ((uintptr_t)d_l2_port & 3u) ||
        ((uintptr_t)d_rx_stats & 7u))
        return NFCS_EINVAL;
    const nfcs::DispatchArgs a{d_arena, arena_bytes, ingress_port, num_ports, n, d_desc, d_action, d_redirect,
                               d_rt_verdict, d_nh, d_l2_port, d_l2_verdict, d_class, d_bypass, d_rx_stats};
    hipStream_t st = pick(c, stream);
    return with_ct_scratch(c, d_rx_stats != nullptr, st,
                           [&](uint64_t* ct) { return nfcs::launch_ingress_dispatch(c->di, f->dev, a, ct, st); });
}

NFCS_API int nfcs_egress_acl_items_host(const nfcs_aclset* s, const uint8_t* arena, uint64_t arena_bytes,
                                        const nfcs_desc* desc, uint32_t n, uint32_t* port, const uint32_t* item_src,
                                        const uint8_t* bypass, uint32_t n_src, uint8_t* action, uint32_t* rule,
                                        uint32_t* redirect, uint32_t* denied_pkts, uint64_t* denied_bytes) {
    if (!s || !s->committed || (!denied_pkts != !denied_bytes) || (!item_src != !bypass)) return NFCS_EINVAL;
    if (n == 0) return NFCS_OK;
    if (!arena || !desc || !port || !action) return NFCS_EINVAL;
    nfcs::aclset_egress(s->t, arena, arena_bytes, desc, n, port, action, rule, redirect, denied_pkts, denied_bytes,
                        item_src, bypass, n_src);
    return NFCS_OK;
}

NFCS_API int nfcs_egress_acl_items_device(nfcs_ctx* c, const nfcs_aclset* s, const uint8_t* d_arena, uint64_t arena_bytes,
                                          const nfcs_desc* d_desc, uint32_t n, uint32_t* d_port,
                                          const uint32_t* d_item_src, const uint8_t* d_bypass, uint32_t n_src,
                                          uint8_t* d_action, uint32_t* d_rule, uint32_t* d_redirect,
                                          uint32_t* d_denied_pkts, uint64_t* d_denied_bytes, void* stream) {
    if (!usable(c, s)) return NFCS_EINVAL;
    if ((!d_denied_pkts != !d_denied_bytes) || (!d_item_src != !d_bypass)) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc || !d_port || !d_action || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    if (((uintptr_t)d_port & 3u) || ((uintptr_t)d_rule & 3u) || ((uintptr_t)d_redirect & 3u) ||
        ((uintptr_t)d_denied_pkts & 3u) || ((uintptr_t)d_denied_bytes & 7u) || ((uintptr_t)d_item_src & 3u))
        return NFCS_EINVAL;
    hipStream_t st = pick(c, stream);
    return with_ct_scratch(c, d_denied_pkts != nullptr, st, [&](uint64_t* ct) {
        return nfcs::launch_egress_acl(c->di, s->dev, d_arena, arena_bytes, d_desc, n, d_port, d_action, d_rule, d_redirect,
                                       d_denied_pkts, d_denied_bytes, ct, st, d_item_src, d_bypass, n_src);
    });
}

}  // extern "C"

namespace {
// nfcs_switch_rx_device's workspace: every intermediate array of the chain, each on a 16-byte boundary.
struct RxWorkspace {
    uint64_t nh, eif, red, l2p, iport, ops, vlan, rt, st, act, l2v, byp, queue, eact, total;
};
RxWorkspace rx_workspace(uint32_t n, uint32_t cap) {
    uint64_t at = 0;
    auto part = [&at](uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 15u) & ~15ull;
        return o;
    };
    RxWorkspace w;
    w.nh = part(4ull * n), w.eif = part(4ull * n), w.red = part(4ull * n), w.l2p = part(4ull * n);
    w.iport = part(4ull * cap), w.ops = part(4ull * cap), w.vlan = part(2ull * n);
    w.rt = part(n), w.st = part(n), w.act = part(n), w.l2v = part(n), w.byp = part(n);
    w.queue = part(cap), w.eact = part(cap);
    w.total = at;
    return w;
}
}  // namespace

extern "C" {

NFCS_API uint64_t nfcs_switch_rx_workspace_bytes(uint32_t n, uint32_t cap) { return rx_workspace(n, cap).total; }

NFCS_API int nfcs_switch_rx_device(nfcs_ctx* c, const nfcs_switch_tables* tb, const nfcs_switch_rx_io* io, void* stream) {
    if (!c || !tb || !io) return NFCS_EINVAL;
    // every table and every argument is tested before the first launch
    if (!usable(c, tb->fib) || !usable(c, tb->fdb) || !usable(c, tb->egress)) return NFCS_EINVAL;
    if ((tb->ingress_acl && !usable(c, tb->ingress_acl)) || (tb->aclset && !usable(c, tb->aclset))) return NFCS_EINVAL;
    if (tb->txq && tb->txq->ctx != c) return NFCS_EINVAL;
    const uint32_t n = io->n, cap = io->cap;
    const RxWorkspace w = rx_workspace(n, cap);
    if (!nfcs::flood_args_ok(io->num_ports, io->arena_bytes, io->copy_base, io->copy_align, n, true, true, true, true, true))
        return NFCS_EINVAL;  // the expand's five input arrays are the workspace's: all given
    if (!io->d_denied_pkts != !io->d_denied_bytes) return NFCS_EINVAL;
    if (tb->txq && tb->txq->dev.keys != tb->egress->dev.keys) return NFCS_EINVAL;  // another egress table's queues
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!io->d_workspace || ((uintptr_t)io->d_workspace & 15u) || io->workspace_bytes < w.total) return NFCS_EINVAL;
    if (!io->d_arena || !io->d_desc || !io->d_totals || ((uintptr_t)io->d_arena & 15u) || ((uintptr_t)io->d_totals & 7u) ||
        ((uintptr_t)io->d_desc & 7u))
        return NFCS_EINVAL;
    if (cap > 0 && (!io->d_item_desc || !io->d_item_port || !io->d_item_src || !io->d_order)) return NFCS_EINVAL;
    if (!io->d_key_start || (tb->egress->dev.keys > 0 && !io->d_depth)) return NFCS_EINVAL;
    if (((uintptr_t)io->d_item_desc & 7u) || ((uintptr_t)io->d_item_port & 3u) || ((uintptr_t)io->d_item_src & 3u) ||
        ((uintptr_t)io->d_order & 3u) || ((uintptr_t)io->d_key_start & 3u) || ((uintptr_t)io->d_key_dropped & 3u) ||
        ((uintptr_t)io->d_depth & 3u) || ((uintptr_t)io->d_denied_pkts & 3u) || ((uintptr_t)io->d_denied_bytes & 7u) ||
        ((uintptr_t)io->d_rx_stats & 7u))
        return NFCS_EINVAL;
    hipStream_t st = pick(c, stream);
    uint8_t* ws = (uint8_t*)io->d_workspace;
    uint32_t *d_nh = (uint32_t*)(ws + w.nh), *d_eif = (uint32_t*)(ws + w.eif), *d_red = (uint32_t*)(ws + w.red);
    uint32_t *d_l2p = (uint32_t*)(ws + w.l2p), *d_iport = (uint32_t*)(ws + w.iport), *d_ops = (uint32_t*)(ws + w.ops);
    uint16_t* d_vlan = (uint16_t*)(ws + w.vlan);
    uint8_t *d_rt = ws + w.rt, *d_st = ws + w.st, *d_act = ws + w.act, *d_l2v = ws + w.l2v, *d_byp = ws + w.byp;
    uint8_t *d_queue = ws + w.queue, *d_eact = ws + w.eact;
    const bool acl = tb->ingress_acl != nullptr;
    const uint64_t frames = io->copy_base;  // the frames lie in [0, copy_base); the copies behind are the egress side's
    // the counter scratch of the dispatch and the egress ACL, before the first launch: without it nothing runs
    const bool counts = io->d_rx_stats || (cap > 0 && tb->aclset && io->d_denied_pkts);
    if (counts) {
        const hipError_t e = acquire_ct(c, st);
        if (e == hipErrorOutOfMemory) return NFCS_ENOMEM;
        NFCS_HIP(e);
    }
    // 1-3: the three decisions (switch.hpp:219-245, 259-301, 305-326)
    NFCS_HIP(nfcs::launch_route_lookup(c->di, tb->fib->dev, io->d_arena, frames, io->d_desc, n, d_nh, d_eif, d_rt, st));
    if (acl)
        NFCS_HIP(nfcs::launch_acl_eval(c->di, tb->ingress_acl->dev, io->d_arena, frames, io->d_desc, n, d_act, nullptr,
                                       d_red, d_nh, st));
    NFCS_HIP(nfcs::launch_l2_lookup(c->di, tb->fdb->dev, io->ingress_port, io->d_arena, frames, io->d_desc, n, d_rt, d_l2p,
                                    d_l2v, d_vlan, nullptr, st));
    // 4: what the switch does between them
    const nfcs::DispatchArgs da{io->d_arena, frames, io->ingress_port, io->num_ports, n, io->d_desc,
                                acl ? d_act : nullptr, acl ? d_red : nullptr, d_rt, d_nh, d_l2p, d_l2v, io->d_class, d_byp,
                                io->d_rx_stats};
    NFCS_HIP(nfcs::launch_ingress_dispatch(c->di, tb->fdb->dev, da, c->ct_ws, st));
    if (io->d_rx_stats) NFCS_HIP(release_ct(c, st));
    // 5: the fused forward
    int rc = l3_forward_device(c, io->d_arena, frames, io->d_desc, d_nh, n, tb->fib->d_table, tb->fib->d_table_n, d_st, st);
    if (rc != NFCS_OK) return rc;
    // 6: the item list and the flood copies
    const nfcs::FloodArgs fa{io->d_arena, io->arena_bytes, io->copy_base, io->copy_align, io->ingress_port, io->num_ports,
                             n, cap, io->d_desc, d_eif, d_st, d_l2p, d_l2v, d_vlan, io->d_item_desc, d_iport,
                             io->d_item_src, io->d_totals};
    rc = with_eq_scratch(c, nfcs::flood_scratch_words(n), st, [&](uint32_t* sc) {
        return nfcs::launch_flood_expand(c->di, tb->fdb->dev, fa, sc, st);
    });
    if (rc != NFCS_OK || cap == 0) return rc;
    // 7-9: process_egress_pipeline over the items (113-139); the plan writes the ports the ACL then edits
    NFCS_HIP(nfcs::launch_egress_plan(c->di, tb->egress->dev, io->d_arena, io->arena_bytes, io->d_item_desc, cap, nullptr,
                                      nullptr, d_iport, io->d_item_port, d_ops, d_queue, st));
    {
        const Shape sh = launch_shape(c, io->arena_bytes, io->d_item_desc, cap, kVlanRule);
        NFCS_HIP(nfcs::launch_vlan(c->di, io->d_arena, io->arena_bytes, io->d_item_desc, cap, d_ops, 0u, nullptr, 0u, nullptr,
                                   st, sh.mean, sh.obs, sh.bits));
    }
    if (tb->aclset) {
        NFCS_HIP(nfcs::launch_egress_acl(c->di, tb->aclset->dev, io->d_arena, io->arena_bytes, io->d_item_desc, cap,
                                         io->d_item_port, d_eact, nullptr, nullptr, io->d_denied_pkts, io->d_denied_bytes,
                                         c->ct_ws, st, io->d_item_src, d_byp, n));
        if (io->d_denied_pkts) NFCS_HIP(release_ct(c, st));
    }
    // 10-11: enqueue_packet (qos_manager.cpp:111-153)
    rc = with_eq_scratch(c, nfcs::egress_scratch_words(cap, tb->egress->dev.keys), st, [&](uint32_t* sc) {
        return nfcs::launch_egress_enqueue(c->di, tb->egress->dev, io->d_item_port, d_queue, cap, io->d_depth, nullptr,
                                           io->d_order, io->d_key_start, io->d_key_dropped, sc, st);
    });
    if (rc != NFCS_OK) return rc;
    if (tb->txq)
        NFCS_HIP(nfcs::launch_txq_append(tb->txq->dev, io->d_order, io->d_key_start, io->d_depth, nullptr, nullptr, cap, st,
                                         io->handle_base));
    return NFCS_OK;
}

NFCS_API int nfcs_update_host(nfcs_ctx* c, uint8_t* h_arena, uint64_t arena_bytes,
                              const nfcs_desc* h_desc, uint32_t n, uint8_t* h_status,
                              uint32_t flags) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!h_arena || !h_desc) return NFCS_EINVAL;
    // Every frame inside the arena fits one staging slot as staged (staged_desc: a frame longer than
    // kFrameRelevantBytes goes as its first kFrameRelevantBytes, round 6; NFCS_EINVAL above 64 MiB
    // before). A frame reaching past the arena is staged as nothing and becomes NFCS_ST_BAD_DESC (the
    // kernel checks it against its chunk), as on the device path. Frames come in any order: a chunk
    // is a run of ascending offsets, so a burst that wraps past its ring's end (round 5; VERDICT r4
    // item 4) is split where an offset drops below its predecessor's, as separate PacketBuffers
    // (packet_buffer.hpp:21-31) never constrain their order either.
    auto frame_end = [&](uint32_t i) -> uint64_t {  // 0: outside the arena; as staged (staged_desc)
        const nfcs_desc d = staged_desc(h_desc[i], arena_bytes);
        const uint64_t o = (uint64_t)d.off16 * 16u;
        const uint64_t e = o + (((uint64_t)d.len + 15u) & ~15ull);
        return e <= arena_bytes ? e : 0;
    };
    bool ordered = true;  // ascending offsets: the chunks' spans are disjoint
    bool any_long = false;  // a frame inside the arena longer than kFrameRelevantBytes (staged_desc)
    for (uint32_t i = 0; i < n; ++i) {
        any_long = any_long || h_desc[i].len > nfcs::kFrameRelevantBytes;
        ordered = ordered && (i == 0 || h_desc[i].off16 >= h_desc[i - 1].off16);
    }
    const uint64_t span = run_span(h_desc, 0, n, arena_bytes);
    int rc = ensure_host_pipeline(c);
    if (rc) return rc;
    const bool pinned = is_pinned(h_arena);
    if (flags & NFCS_HOST_ZERO_COPY) {
        if (!pinned) return NFCS_EINVAL;
        return update_host_zero_copy(c, h_arena, arena_bytes, h_desc, n, h_status, any_long);
    }
    // A pinned arena's burst of at most kZeroCopyAutoBytes of frames (the default, records form) runs
    // zero-copy: the kernel reads its frames in place and stores the checksum bytes straight back,
    // the same bytes the records would carry (round 6, profiles/r06_host_bursts_ab.jsonl: 64 to 16K C1
    // frames 2-18% faster zero-copy than through the copy engines, 64K 3-5% slower)
    // (a 16-byte aligned arena only: the kernel's 16-byte loads address the frames in place)
    const bool aligned = ((uintptr_t)h_arena & 15u) == 0;
    if (pinned && aligned && !(flags & NFCS_HOST_FRAMES) && span <= kZeroCopyAutoBytes)
        return update_host_zero_copy(c, h_arena, arena_bytes, h_desc, n, h_status, any_long);
    // default: frames H2D and only the 8-byte patch records D2H (kUpdateRecords: the staged
    // frames are not written), applied here; whole frames back only on request (NFCS_HOST_FRAMES:
    // kUpdateAuto on the staged frames, the slot's patch buffer as the deferred-store workspace)
    const bool patch_only = !(flags & NFCS_HOST_FRAMES);
    // Chunk size: a burst is cut into ~4 chunks (at least kMinChunk bytes, at most a staging slot)
    // so that its host copy, H2D copy, kernel, D2H copy and patch application overlap across the
    // two slots even when it would fit one slot (16K C1 frames: pinned 583 -> 559 µs, pageable
    // 979 -> 710 µs; 64K: 2267 -> 1992 / 3133 -> 2273 µs). Whole frames back from a pinned arena
    // keep slot-sized chunks (4 chunks measured slower there: 64K 3.13 -> 3.59 ms).
    const uint64_t chunk_target = (!patch_only && pinned) ? nfcs_ctx::kStageBytes : chunk_bytes(span);

    struct Chunk { uint32_t i0, i1; uint64_t base, bytes; bool used; };
    Chunk slot[nfcs_ctx::kSlots] = {};
    hipError_t e = hipSuccess;
    // finish a slot: wait for its D2H, then apply patches / copy frames / copy statuses (only
    // while no error has occurred; after one the slot is only drained)
    auto finish = [&](int s) {
        Chunk& k = slot[s];
        if (!k.used) return;
        k.used = false;
        const hipError_t f = wait_slot(c, s, c->done[s]);
        if (e == hipSuccess) e = f;
        if (e != hipSuccess) return;
        const uint32_t m = k.i1 - k.i0;
        if (patch_only) {
            // each record writes into another frame's header line, which the DMA read but the
            // CPU has not cached: prefetch the line kPf packets ahead so the misses overlap; large
            // chunks over the workers
            const nfcs_patch* pq = c->h_patch[s];
            const int np = std::min<int>(c->workers.size() + 1, std::max<uint32_t>(1, m / kPatchFramesPerThread));
            c->workers.run(np, [&](int t) {
                const uint32_t j0 = (uint32_t)((uint64_t)m * t / np), j1 = (uint32_t)((uint64_t)m * (t + 1) / np);
                constexpr uint32_t kPf = 16;
                for (uint32_t j = j0; j < j1; ++j) {
                    if (j + kPf < j1) {
                        const nfcs_patch& q = pq[j + kPf];
                        const uint32_t o = q.ip_off != NFCS_PATCH_NONE ? q.ip_off : q.l4_off;
                        const uint64_t a = (uint64_t)h_desc[k.i0 + j + kPf].off16 * 16u + (o & 0xFFC0u);
                        if (a < arena_bytes) __builtin_prefetch(h_arena + a, 1, 0);
                    }
                    const nfcs_patch& pt = pq[j];
                    if (!frame_end(k.i0 + j)) continue;
                    uint8_t* f = h_arena + (uint64_t)h_desc[k.i0 + j].off16 * 16u;
                    if (pt.ip_off != NFCS_PATCH_NONE) { f[pt.ip_off] = pt.ip[0]; f[pt.ip_off + 1] = pt.ip[1]; }
                    if (pt.l4_off != NFCS_PATCH_NONE) { f[pt.l4_off] = pt.l4[0]; f[pt.l4_off + 1] = pt.l4[1]; }
                }
            });
        } else if (ordered && !pinned) {
            par_memcpy(c, h_arena + k.base, c->h_arena[s], k.bytes);
        } else if (!ordered) {
            // Frames in any order: a chunk's span can hold frames of other chunks, staged before an
            // earlier chunk wrote them back, so only the chunk's own frames are copied back (from
            // the slot, where the frames came back also for a pinned arena)
            const int np = m >= 16384 ? c->workers.size() + 1 : 1;
            c->workers.run(np, [&](int t) {
                for (uint32_t j = (uint32_t)((uint64_t)m * t / np); j < (uint32_t)((uint64_t)m * (t + 1) / np); ++j) {
                    const uint32_t q = k.i0 + j;
                    if (!frame_end(q)) continue;
                    const uint64_t o = (uint64_t)h_desc[q].off16 * 16u;
                    memcpy(h_arena + o, c->h_arena[s] + (o - k.base), staged_desc(h_desc[q], arena_bytes).len);
                }
            });
        }
        if (h_status) memcpy(h_status + k.i0, c->h_status[s], m);
    };

    uint32_t i = 0;
    int s = 0;
    while (i < n && e == hipSuccess) {
        // next chunk: packets [i, i1) in ascending arena order whose in-arena frames fit one
        // staging slot (a ring wrap closes the chunk: the next one starts at the lower offset)
        const uint64_t base = std::min<uint64_t>((uint64_t)h_desc[i].off16 * 16u, arena_bytes);
        uint32_t i1 = i;
        uint64_t end = base;
        while (i1 < n && i1 - i < c->stage_pkts) {
            if (i1 > i && h_desc[i1].off16 < h_desc[i1 - 1].off16) break;
            const uint64_t fe = frame_end(i1);
            const uint64_t ne = std::max(end, fe);
            if (ne - base > c->stage_bytes) break;  // i1 > i: a single frame always fits (above)
            if (i1 > i && ne - base > chunk_target) break;
            end = ne;
            ++i1;
        }
        // With patch records back, the slot's host arena and descriptors are free again once chunk
        // k-2 has been copied in (`staged`), so chunk k's staging copy runs before chunk k-2's
        // patches are applied and beside chunk k-1's transfer (round 5); with whole frames back the
        // slot's arena receives them, and chunk k-2 is finished first
        if (!patch_only) {
            finish(s);
        } else if (slot[s].used) {
            e = wait_slot(c, s, c->staged[s]);
        }
        if (e != hipSuccess) break;
        const uint32_t m = i1 - i;
        const uint64_t bytes = end - base;
        const uint8_t* src = h_arena + base;
        // a direct chunk (records back, small): no DMA; the kernel reads a pinned arena in place
        uint8_t* zsrc = nullptr;
        if (patch_only && c->z_block[s] && bytes <= kDirectChunkBytes && (!pinned || aligned)) {
            if (pinned) {
                void* dp = nullptr;
                if (hipHostGetDevicePointer(&dp, h_arena, 0) == hipSuccess) zsrc = static_cast<uint8_t*>(dp) + base;
                else (void)hipGetLastError();
            } else {
                zsrc = zdev(c, s, c->h_arena[s]);
            }
        }
        if (!pinned) {
            par_memcpy(c, c->h_arena[s], src, bytes);
            src = c->h_arena[s];
        }
        stage_descs(c->h_desc[s], h_desc + i, m, arena_bytes, any_long);
        if (patch_only) {
            finish(s);  // chunk k-2's records and statuses are read out before chunk k's land
            if (e != hipSuccess) break;
        }
        hipStream_t st = c->hs[s];
        if (zsrc) {
            e = nfcs::launch_update(c->di, zsrc, bytes ? bytes : 16, zdev(c, s, c->h_desc[s]), m, (uint32_t)(base >> 4),
                                    h_status ? zdev(c, s, c->h_status[s]) : nullptr, zdev(c, s, c->h_patch[s]),
                                    nullptr, nfcs::kUpdateRecords, st, 0, {}, done_req(c, s));
            if (e == hipSuccess) e = hipEventRecord(c->staged[s], st);  // the kernel read the slot
            if (e == hipSuccess) e = hipEventRecord(c->done[s], st);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(st);
                break;
            }
            slot[s] = {i, i1, base, bytes, true};
            i = i1;
            s ^= 1;
            continue;
        }
        event_wait(c, s);
        e = hipMemcpyAsync(c->d_desc[s], c->h_desc[s], (size_t)m * sizeof(nfcs_desc),
                           hipMemcpyHostToDevice, st);
        if (e == hipSuccess && bytes)
            e = hipMemcpyAsync(c->d_arena[s], src, bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(c->staged[s], st);
        if (e == hipSuccess)
            e = nfcs::launch_update(c->di, c->d_arena[s], bytes, c->d_desc[s], m, (uint32_t)(base >> 4),
                                    c->d_status[s], patch_only ? c->d_patch[s] : nullptr,
                                    patch_only ? nullptr : c->d_patch[s],
                                    patch_only ? nfcs::kUpdateRecords : nfcs::kUpdateAuto, st);
        if (e == hipSuccess) {
            if (patch_only)
                e = hipMemcpyAsync(c->h_patch[s], c->d_patch[s], (size_t)m * sizeof(nfcs_patch),
                                   hipMemcpyDeviceToHost, st);
            else if (bytes)
                e = hipMemcpyAsync(pinned && ordered ? h_arena + base : c->h_arena[s], c->d_arena[s], bytes,
                                   hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess && h_status)
            e = hipMemcpyAsync(c->h_status[s], c->d_status[s], m, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(c->done[s], st);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);  // whatever was queued on this slot has finished
            break;
        }
        slot[s] = {i, i1, base, bytes, true};
        i = i1;
        s ^= 1;
    }
    finish(s);  // drain both slots, also after an error
    finish(s ^ 1);
    if (e != hipSuccess) return hip_fail(e);
    return NFCS_OK;
}

NFCS_API int nfcs_update_host_frames(nfcs_ctx* c, uint8_t* const* frames, const uint32_t* lens, uint32_t n,
                                     uint8_t* h_status, uint32_t flags) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!frames || !lens || flags != 0) return NFCS_EINVAL;
    int rc = ensure_host_pipeline(c);
    if (rc) return rc;
    // a NULL frame is empty; a frame longer than kFrameRelevantBytes is staged as its first
    // kFrameRelevantBytes bytes, which changes nothing (nfcs.h): so no frame outgrows a staging slot
    auto flen = [&](uint32_t i) -> uint64_t { return frames[i] ? std::min(lens[i], nfcs::kFrameRelevantBytes) : 0u; };
    auto pad = [](uint64_t len) { return (len + 15u) & ~15ull; };
    const int parts = c->workers.size() + 1;
    // the burst's padded bytes (every frame fits one staging slot: checked anyway), over the workers
    // for large bursts (no serial pass over the burst on the caller's thread)
    uint64_t chunk_target = 0;
    {
        constexpr int kMaxParts = 65;
        uint64_t tot[kMaxParts] = {};
        bool bad[kMaxParts] = {};
        const int np = n >= 65536 ? std::min(parts, kMaxParts) : 1;
        c->workers.run(np, [&](int t) {
            const uint32_t j0 = (uint32_t)((uint64_t)n * t / np), j1 = (uint32_t)((uint64_t)n * (t + 1) / np);
            uint64_t sum = 0;
            bool b = false;
            for (uint32_t j = j0; j < j1; ++j) {
                const uint64_t l = flen(j);
                b |= l > nfcs_ctx::kStageBytes;
                sum += pad(l);
            }
            tot[t] = sum;
            bad[t] = b;
        });
        uint64_t total = 0;
        for (int t = 0; t < np; ++t) {
            if (bad[t]) return NFCS_EINVAL;
            total += tot[t];
        }
        // chunks of ~a quarter of the burst (at least 4 MiB, at most a staging slot), as
        // nfcs_update_host cuts them
        chunk_target = chunk_bytes(total);
    }

    // The pipeline over the two slots, per chunk k in slot s: wait until chunk k-2's frames and
    // descriptors have been copied in (`staged`: the slot's host arena is free again — not for its
    // kernel and records, round 5), lay out chunk k's descriptors, gather its frames (the workers),
    // then finish chunk k-2 (its records: checksum bytes written into the frames) and queue chunk
    // k's copies, kernel and record copy. So the gather of chunk k runs beside the copy of chunk k-1.
    struct Chunk { uint32_t i0, i1; bool used; };
    Chunk slot[nfcs_ctx::kSlots] = {};
    hipError_t e = hipSuccess;
    // finish a slot: wait for its records, then write each frame's checksum bytes in place (ip
    // field first, then l4: the reference's order, which also reproduces IHL < 5 overlaps) and copy
    // its statuses; after an error the slot is only drained
    auto finish = [&](int s) {
        Chunk& k = slot[s];
        if (!k.used) return;
        k.used = false;
        const hipError_t f = wait_slot(c, s, c->done[s]);
        if (e == hipSuccess) e = f;
        if (e != hipSuccess) return;
        const uint32_t m = k.i1 - k.i0;
        const nfcs_patch* pt = c->h_patch[s];
        const int np = std::min<int>(parts, std::max<uint32_t>(1, m / kPatchFramesPerThread));
        c->workers.run(np, [&](int t) {
            const uint32_t j0 = (uint32_t)((uint64_t)m * t / np), j1 = (uint32_t)((uint64_t)m * (t + 1) / np);
            constexpr uint32_t kPf = 16;  // the header lines of frames kPf ahead: their misses overlap
            for (uint32_t j = j0; j < j1; ++j) {
                if (j + kPf < j1 && frames[k.i0 + j + kPf]) __builtin_prefetch(frames[k.i0 + j + kPf] + 32, 1, 0);
                uint8_t* fr = frames[k.i0 + j];
                if (!fr) continue;
                if (pt[j].ip_off != NFCS_PATCH_NONE) { fr[pt[j].ip_off] = pt[j].ip[0]; fr[pt[j].ip_off + 1] = pt[j].ip[1]; }
                if (pt[j].l4_off != NFCS_PATCH_NONE) { fr[pt[j].l4_off] = pt[j].l4[0]; fr[pt[j].l4_off + 1] = pt[j].l4[1]; }
            }
        });
        if (h_status) memcpy(h_status + k.i0, c->h_status[s], m);
    };

    uint32_t i = 0;
    int s = 0;
    while (i < n && e == hipSuccess) {
        if (slot[s].used) {  // chunk k-2's copies in are done: its arena and descriptors are free
            e = wait_slot(c, s, c->staged[s]);
            if (e != hipSuccess) break;
        }
        // next chunk: packets [i, i1), their 16-byte padded frames within chunk_target bytes (at
        // least one) and the slot's descriptor room, laid out back to back in the slot
        nfcs_desc* hd = c->h_desc[s];
        uint32_t i1 = i;
        uint64_t bytes = 0;
        while (i1 < n && i1 - i < c->stage_pkts) {
            const uint64_t l = flen(i1), b = bytes + pad(l);
            if (i1 > i && b > chunk_target) break;
            hd[i1 - i] = nfcs_desc{(uint32_t)(bytes >> 4), (uint32_t)l};
            bytes = b;
            ++i1;
        }
        const uint32_t m = i1 - i;
        uint8_t* dst = c->h_arena[s];
        const int ng = (int)std::min<uint64_t>(parts, std::max<uint64_t>(1, bytes / kCopyBytesPerThread));
        c->workers.run(ng, [&](int t) {
            const uint32_t j0 = (uint32_t)((uint64_t)m * t / ng), j1 = (uint32_t)((uint64_t)m * (t + 1) / ng);
            constexpr uint32_t kPf = 4;  // the first lines of the frame kPf ahead: its misses overlap this copy
            for (uint32_t j = j0; j < j1; ++j) {
                if (j + kPf < j1 && frames[i + j + kPf]) {
                    __builtin_prefetch(frames[i + j + kPf], 0, 0);
                    __builtin_prefetch(frames[i + j + kPf] + 64, 0, 0);
                    __builtin_prefetch(frames[i + j + kPf] + 128, 0, 0);
                }
                const uint64_t len = hd[j].len, o = (uint64_t)hd[j].off16 * 16u;
                // the slot's 16-byte padding zeroed: the kernel reads whole 16-byte chunks
                if (len) stream_copy(dst + o, frames[i + j], len, true);
            }
            nt_fence();
        });
        finish(s);  // chunk k-2: its records and statuses are read out of the slot before chunk k's land
        if (e != hipSuccess) break;
        hipStream_t st = c->hs[s];
        if (c->z_block[s] && bytes <= kDirectChunkBytes) {
            // a direct chunk: the kernel reads the gathered frames and descriptors in the pinned slot
            // and writes records and statuses there; no DMA (kDirectChunkBytes)
            e = nfcs::launch_update(c->di, zdev(c, s, dst), bytes ? bytes : 16, zdev(c, s, hd), m, 0u,
                                    h_status ? zdev(c, s, c->h_status[s]) : nullptr, zdev(c, s, c->h_patch[s]),
                                    nullptr, nfcs::kUpdateRecords, st, 0, {}, done_req(c, s));
            if (e == hipSuccess) e = hipEventRecord(c->staged[s], st);
        } else {
            event_wait(c, s);
            e = hipMemcpyAsync(c->d_desc[s], hd, (size_t)m * sizeof(nfcs_desc), hipMemcpyHostToDevice, st);
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(c->d_arena[s], dst, bytes, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipEventRecord(c->staged[s], st);
            if (e == hipSuccess)
                e = nfcs::launch_update(c->di, c->d_arena[s], bytes ? bytes : 16, c->d_desc[s], m, 0u, c->d_status[s],
                                        c->d_patch[s], nullptr, nfcs::kUpdateRecords, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(c->h_patch[s], c->d_patch[s], (size_t)m * sizeof(nfcs_patch), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && h_status) e = hipMemcpyAsync(c->h_status[s], c->d_status[s], m, hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess) e = hipEventRecord(c->done[s], st);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);  // whatever was queued on this slot has finished
            break;
        }
        slot[s] = {i, i1, true};
        i = i1;
        s ^= 1;
    }
    finish(s);  // drain both slots, also after an error
    finish(s ^ 1);
    if (e != hipSuccess) return hip_fail(e);
    return NFCS_OK;
}

NFCS_API int nfcs_shard_bytes(const nfcs_desc* h_desc, uint32_t n, uint32_t parts, uint32_t* bounds) {
    if (!bounds || parts == 0 || (n && !h_desc)) return NFCS_EINVAL;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += h_desc[i].len;
    // bounds[p] = the first packet at which the running byte count reaches p * total / parts, so
    // every boundary lies within one frame of its ideal position
    uint32_t i = 0;
    uint64_t run = 0;
    bounds[0] = 0;
    for (uint32_t p = 1; p < parts; ++p) {
        const unsigned __int128 t = (unsigned __int128)total * p;
        const uint64_t target = (uint64_t)(t / parts) + (t % parts != 0);
        while (i < n && run < target) run += h_desc[i++].len;
        bounds[p] = i;
    }
    bounds[parts] = n;
    return NFCS_OK;
}

NFCS_API int nfcs_layout_config(int config, uint64_t seed, uint64_t first_index, uint32_t n,
                                uint32_t align, nfcs_desc* h_desc, uint64_t* arena_bytes) {
    if (config < 0 || config > 3 || align < 16 || (align & 15u)) return NFCS_EINVAL;
    uint64_t off = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = nfcs::config_len(config, seed, first_index + i);
        if ((off >> 4) > 0xFFFFFFFFull) return NFCS_EINVAL;
        if (h_desc) h_desc[i] = nfcs_desc{(uint32_t)(off >> 4), len};
        off += ((uint64_t)len + align - 1) / align * align;
    }
    if (arena_bytes) *arena_bytes = off;
    return NFCS_OK;
}

NFCS_API int nfcs_gen_config_device(nfcs_ctx* c, int config, uint64_t seed, uint64_t first,
                                    uint32_t n, uint8_t* d_arena, uint64_t arena_bytes,
                                    const nfcs_desc* d_desc, void* stream) {
    if (!c || config < 0 || config > 3) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0) return NFCS_OK;
    if (!d_arena || !d_desc) return NFCS_EINVAL;
    // padding between aligned frame starts is zeroed too, so the arena is fully defined
    NFCS_HIP(hipMemsetAsync(d_arena, 0, arena_bytes, pick(c, stream)));
    NFCS_HIP(nfcs::launch_gen_config(c->di, config, seed, first, n, d_arena, arena_bytes, d_desc,
                                     pick(c, stream)));
    return NFCS_OK;
}

NFCS_API int nfcs_stale_every_device(nfcs_ctx* c, uint8_t* d_arena, uint64_t arena_bytes,
                                     const nfcs_desc* d_desc, uint32_t n, uint32_t every, void* stream) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    if (n == 0 || every == 0) return NFCS_OK;
    if (!d_arena || !d_desc) return NFCS_EINVAL;
    NFCS_HIP(nfcs::launch_stale_every(d_arena, arena_bytes, d_desc, n, every, pick(c, stream)));
    return NFCS_OK;
}

NFCS_API int nfcs_digest_device(nfcs_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes,
                                const nfcs_desc* d_desc, uint32_t n, uint64_t first,
                                uint64_t* h_digest, void* stream) {
    if (!c || !h_digest) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipStream_t st = pick(c, stream);
    NFCS_HIP(hipMemsetAsync(c->d_digest, 0, sizeof(uint64_t), st));
    if (n) {
        if (!d_arena || !d_desc) return NFCS_EINVAL;
        const hipError_t e = acquire_ct(c, st);
        if (e == hipErrorOutOfMemory) return NFCS_ENOMEM;
        NFCS_HIP(e);
        NFCS_HIP(nfcs::launch_digest(c->di, d_arena, arena_bytes, d_desc, n, first, c->d_digest, c->ct_ws, st));
        NFCS_HIP(release_ct(c, st));
    }
    NFCS_HIP(hipMemcpyAsync(h_digest, c->d_digest, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    NFCS_HIP(hipStreamSynchronize(st));
    return NFCS_OK;
}

NFCS_API int nfcs_device_alloc(nfcs_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return NFCS_ENOMEM; }
    NFCS_HIP(e);
    return NFCS_OK;
}
NFCS_API int nfcs_device_free(nfcs_ctx* c, void* p) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    NFCS_HIP(hipFree(p));
    return NFCS_OK;
}
NFCS_API int nfcs_host_alloc(nfcs_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return NFCS_ENOMEM; }
    NFCS_HIP(e);
    return NFCS_OK;
}
NFCS_API int nfcs_host_free(nfcs_ctx* c, void* p) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    NFCS_HIP(hipHostFree(p));
    return NFCS_OK;
}
NFCS_API int nfcs_memcpy_h2d(nfcs_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    NFCS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    NFCS_HIP(hipStreamSynchronize(c->stream));
    return NFCS_OK;
}
NFCS_API int nfcs_memcpy_d2h(nfcs_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    NFCS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    NFCS_HIP(hipStreamSynchronize(c->stream));
    return NFCS_OK;
}
NFCS_API int nfcs_stream_sync(nfcs_ctx* c, void* stream) {
    if (!c) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    NFCS_HIP(hipStreamSynchronize(pick(c, stream)));
    return NFCS_OK;
}


NFCS_API int nfcs_time_update_device(nfcs_ctx* c, uint8_t* d_arena, uint64_t arena_bytes,
                                     const nfcs_desc* d_desc, uint32_t n, uint8_t* d_status,
                                     int iters, void* stream, float* ms) {
    if (!c || !ms || iters <= 0) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipStream_t st = pick(c, stream);
    if (!d_arena || !d_desc || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    NFCS_HIP(hipEventRecord(c->ev0, st));
    for (int it = 0; it < iters; ++it) {
        const int rc = update_device(c, d_arena, arena_bytes, d_desc, n, d_status, nullptr, st);
        if (rc) return rc;
    }
    NFCS_HIP(hipEventRecord(c->ev1, st));
    NFCS_HIP(hipEventSynchronize(c->ev1));
    NFCS_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return NFCS_OK;
}

NFCS_API int nfcs_time_update_batches(nfcs_ctx* c, uint32_t batches, uint8_t* const* d_arenas,
                                      const uint64_t* arena_bytes, const nfcs_desc* const* d_descs,
                                      uint32_t n, int iters, void* stream, float* ms) {
    if (!c || !ms || iters <= 0 || batches == 0 || !d_arenas || !arena_bytes || !d_descs) return NFCS_EINVAL;
    for (uint32_t b = 0; b < batches; ++b)
        if (!d_arenas[b] || !d_descs[b] || ((uintptr_t)d_arenas[b] & 15u)) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipStream_t st = pick(c, stream);
    NFCS_HIP(hipEventRecord(c->ev0, st));
    for (int it = 0; it < iters; ++it) {
        const uint32_t b = (uint32_t)it % batches;
        const int rc = update_device(c, d_arenas[b], arena_bytes[b], d_descs[b], n, nullptr, nullptr, st);
        if (rc) return rc;
    }
    NFCS_HIP(hipEventRecord(c->ev1, st));
    NFCS_HIP(hipEventSynchronize(c->ev1));
    NFCS_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return NFCS_OK;
}

NFCS_API int nfcs_time_l3_forward_device(nfcs_ctx* c, uint8_t* d_arena, uint64_t arena_bytes,
                                         const nfcs_desc* d_desc, const uint32_t* d_nh,
                                         uint32_t n, const nfcs_nexthop* d_table, uint32_t table_n,
                                         uint8_t* d_status, int iters, void* stream, float* ms) {
    if (!c || !ms || iters <= 0 || !d_arena || !d_desc || !d_nh) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipStream_t st = pick(c, stream);
    NFCS_HIP(hipEventRecord(c->ev0, st));
    for (int it = 0; it < iters; ++it) {
        const int rc = l3_forward_device(c, d_arena, arena_bytes, d_desc, d_nh, n, d_table, table_n,
                                         d_status, st);
        if (rc) return rc;
    }
    NFCS_HIP(hipEventRecord(c->ev1, st));
    NFCS_HIP(hipEventSynchronize(c->ev1));
    NFCS_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return NFCS_OK;
}

NFCS_API int nfcs_time_vlan_device(nfcs_ctx* c, uint8_t* d_arena, uint64_t arena_bytes,
                                   nfcs_desc* d_desc, uint32_t n, uint32_t op_all,
                                   uint32_t op_alt, uint32_t cap_all, uint8_t* d_status, int iters,
                                   void* stream, float* ms) {
    if (!c || !ms || iters <= 0 || !d_arena || !d_desc) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipStream_t st = pick(c, stream);
    NFCS_HIP(hipEventRecord(c->ev0, st));
    for (int it = 0; it < iters; ++it) {
        const Shape sh = launch_shape(c, arena_bytes, d_desc, n, kVlanRule);
        NFCS_HIP(nfcs::launch_vlan(c->di, d_arena, arena_bytes, d_desc, n, nullptr,
                                   (it & 1) ? op_alt : op_all, nullptr, cap_all, d_status, st,
                                   sh.mean, sh.obs, sh.bits));
    }
    NFCS_HIP(hipEventRecord(c->ev1, st));
    NFCS_HIP(hipEventSynchronize(c->ev1));
    NFCS_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return NFCS_OK;
}

NFCS_API int nfcs_time_flow_keys_device(nfcs_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes,
                                        const nfcs_desc* d_desc, uint32_t n, nfcs_flow_key* d_keys,
                                        uint32_t* d_hash, int iters, void* stream, float* ms) {
    if (!c || !ms || iters <= 0 || !d_arena || !d_desc) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipStream_t st = pick(c, stream);
    NFCS_HIP(hipEventRecord(c->ev0, st));
    for (int it = 0; it < iters; ++it)
        NFCS_HIP(nfcs::launch_flow_keys(c->di, d_arena, arena_bytes, d_desc, n, d_keys, d_hash, st));
    NFCS_HIP(hipEventRecord(c->ev1, st));
    NFCS_HIP(hipEventSynchronize(c->ev1));
    NFCS_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return NFCS_OK;
}

NFCS_API int nfcs_time_stream_read(nfcs_ctx* c, const uint8_t* d_buf, uint64_t bytes, int form, int iters,
                                   void* stream, float* ms) {
    if (!c || !ms || iters <= 0 || !d_buf || form < 0 || form > 5 || ((uintptr_t)d_buf & 15u))
        return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipStream_t st = pick(c, stream);
    unsigned long long* sink = reinterpret_cast<unsigned long long*>(c->d_digest);
    NFCS_HIP(hipEventRecord(c->ev0, st));
    for (int it = 0; it < iters; ++it) NFCS_HIP(nfcs::launch_stream_read(d_buf, bytes, form, sink, st));
    NFCS_HIP(hipEventRecord(c->ev1, st));
    NFCS_HIP(hipEventSynchronize(c->ev1));
    NFCS_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return NFCS_OK;
}

NFCS_API int nfcs_time_frames_read(nfcs_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes,
                                   const nfcs_desc* d_desc, uint32_t n, int iters, void* stream, float* ms) {
    if (!c || !ms || iters <= 0 || !d_arena || !d_desc || ((uintptr_t)d_arena & 15u)) return NFCS_EINVAL;
    DeviceGuard dg_(c->di.device);  // the context's device on this thread, restored on return
    if (dg_.err != hipSuccess) return hip_fail(dg_.err);
    hipStream_t st = pick(c, stream);
    unsigned long long* sink = reinterpret_cast<unsigned long long*>(c->d_digest);
    NFCS_HIP(hipEventRecord(c->ev0, st));
    for (int it = 0; it < iters; ++it) NFCS_HIP(nfcs::launch_frames_read(d_arena, arena_bytes, d_desc, n, sink, st));
    NFCS_HIP(hipEventRecord(c->ev1, st));
    NFCS_HIP(hipEventSynchronize(c->ev1));
    NFCS_HIP(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return NFCS_OK;
}

}  // extern "C"
