// C ABI: RCCL collectives.
// Part of the host runtime of libexacto_hip.so; the shared types and helpers are in runtime.hpp.
#include "runtime.hpp"

using namespace exacto;

// ============================================================== RCCL collectives
//
// Keys are made once and broadcast over xGMI to every GPU (the reference builds them on one host,
// keygen.rs:123-209); the limbs of a split dbfv_mul are gathered (never summed: an RCCL sum of
// residues would overflow mod q).  librccl is opened at first use (dlopen of librccl.so.1, or
// EXACTO_RCCL_LIB), so a process that already loaded RCCL (torch) shares that instance and the
// library has no link-time dependency on it.  Communicators are plain ncclComm_t handles, passed as
// void*: made here (exacto_rccl_comm_init) or by the caller's own RCCL.

#include <rccl/rccl.h>

namespace {
struct Rccl {
    bool ok = false;
    std::string why;
    ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*comm_count)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*comm_user_rank)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
    // optional (deadline handling): a communicator whose collective missed its deadline is aborted
    ncclResult_t (*comm_abort)(ncclComm_t) = nullptr;
    ncclResult_t (*async_error)(ncclComm_t, ncclResult_t*) = nullptr;
};

const Rccl& rccl() {
    static const Rccl r = [] {
        Rccl x;
        const char* env = getenv("EXACTO_RCCL_LIB");
        void* h = dlopen(env ? env : "librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) { x.why = std::string("cannot open RCCL: ") + dlerror(); return x; }
        bool all = true;
        auto sym = [&](auto& f, const char* name) {
            f = reinterpret_cast<std::remove_reference_t<decltype(f)>>(dlsym(h, name));
            all &= f != nullptr;
        };
        sym(x.get_unique_id, "ncclGetUniqueId");
        sym(x.comm_init_rank, "ncclCommInitRank");
        sym(x.comm_destroy, "ncclCommDestroy");
        sym(x.comm_count, "ncclCommCount");
        sym(x.comm_user_rank, "ncclCommUserRank");
        sym(x.broadcast, "ncclBroadcast");
        sym(x.all_gather, "ncclAllGather");
        sym(x.error_string, "ncclGetErrorString");
        x.ok = all;
        x.comm_abort = reinterpret_cast<decltype(x.comm_abort)>(dlsym(h, "ncclCommAbort"));
        x.async_error = reinterpret_cast<decltype(x.async_error)>(dlsym(h, "ncclCommGetAsyncError"));
        if (!all) x.why = "RCCL library lacks a required symbol";
        return x;
    }();
    return r;
}
}  // namespace

#define RCCL_TRY(x)                                                                                      \
    do {                                                                                                 \
        const ncclResult_t r_ = (x);                                                                     \
        if (r_ != ncclSuccess)                                                                           \
            return fail(EXACTO_ERR_HIP, std::string("RCCL error: ") + rccl().error_string(r_) + " (" #x ")"); \
    } while (0)

static int rccl_ready() {
    if (!rccl().ok) return fail(EXACTO_ERR_HIP, "RCCL error: " + rccl().why);
    return 0;
}

extern "C" int exacto_rccl_unique_id(uint8_t* id) {
    if (!id) return invalid_param("null id buffer");
    if (int e = rccl_ready()) return e;
    ncclUniqueId u;
    RCCL_TRY(rccl().get_unique_id(&u));
    std::memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
    return 0;
}

// Deadline of the blocking RCCL steps (communicator init, the agreement all-gather, exacto_rccl_sync):
// $EXACTO_RCCL_TIMEOUT_S seconds (default 300; 0 = wait forever).  A rank that never joins makes the
// others fail with EXACTO_ERR_HIP "RCCL error: ... timed out" instead of blocking their process for
// good (the driver's 8-GPU run has one time limit for everything).
static double rccl_timeout_s() {
    const char* e = getenv("EXACTO_RCCL_TIMEOUT_S");
    return e ? atof(e) : 300.0;
}

// Communicators aborted after a missed deadline: RCCL has freed them, so destroy must not touch them.
static std::mutex g_aborted_mu;
static std::set<void*> g_aborted;

static int rccl_abort_timeout(void* comm, const std::string& what, double secs) {
    if (rccl().comm_abort) {
        (void)rccl().comm_abort((ncclComm_t)comm);
        std::lock_guard<std::mutex> g(g_aborted_mu);
        g_aborted.insert(comm);
    }
    return fail(EXACTO_ERR_HIP, "RCCL error: " + what + " timed out after " + std::to_string((int)secs) +
                                    " s (a rank did not join); communicator aborted");
}

// Waits for the context stream (the collectives enqueued on it) with the deadline: polls hipStreamQuery
// and the communicator's asynchronous error.  On expiry the communicator is aborted (RCCL then stops its
// kernels) and the call fails; it never returns with a collective still blocking the stream silently.
static int rccl_stream_wait(exacto_ctx* c, void* comm, const char* what) {
    const double lim = rccl_timeout_s();
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0;; ++it) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) return fail(EXACTO_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(q) + " (" + what + ")");
        if (rccl().async_error) {
            ncclResult_t ae = ncclSuccess;
            if (rccl().async_error((ncclComm_t)comm, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress)
                return fail(EXACTO_ERR_HIP, std::string("RCCL error: ") + rccl().error_string(ae) + " (" + what + ")");
        }
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (lim > 0 && el > lim) return rccl_abort_timeout(comm, what, lim);
        std::this_thread::sleep_for(std::chrono::microseconds(it < 100 ? 20 : 1000));
    }
}

extern "C" int exacto_rccl_comm_init(void** comm, int nranks, const uint8_t* id, int rank, int device) {
    if (!comm || !id) return invalid_param("null argument");
    if (nranks < 1 || rank < 0 || rank >= nranks) return invalid_param("rank out of range");
    if (int e = rccl_ready()) return e;
    HIP_TRY(hipSetDevice(device));
    ncclUniqueId u;
    std::memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
    // ncclCommInitRank blocks until every rank has joined: it runs on a helper thread so that the
    // caller's wait has a deadline.  On expiry the helper is left behind (it holds only its own copy
    // of the arguments) and the call fails; the caller is expected to end the process.
    struct InitState {
        std::mutex mu;
        std::condition_variable cv;
        bool done = false;
        ncclResult_t r = ncclSuccess;
        ncclComm_t cm = nullptr;
    };
    auto st = std::make_shared<InitState>();
    std::thread([st, nranks, u, rank, device] {
        (void)hipSetDevice(device);
        ncclComm_t cm = nullptr;
        const ncclResult_t r = rccl().comm_init_rank(&cm, nranks, u, rank);
        std::lock_guard<std::mutex> g(st->mu);
        st->r = r;
        st->cm = cm;
        st->done = true;
        st->cv.notify_all();
    }).detach();
    const double lim = rccl_timeout_s();
    std::unique_lock<std::mutex> lk(st->mu);
    if (lim > 0) {
        if (!st->cv.wait_for(lk, std::chrono::duration<double>(lim), [&] { return st->done; }))
            return fail(EXACTO_ERR_HIP, "RCCL error: ncclCommInitRank timed out after " + std::to_string((int)lim) +
                                            " s (a rank did not join)");
    } else {
        st->cv.wait(lk, [&] { return st->done; });
    }
    if (st->r != ncclSuccess)
        return fail(EXACTO_ERR_HIP, std::string("RCCL error: ") + rccl().error_string(st->r) + " (ncclCommInitRank)");
    *comm = st->cm;
    return 0;
}

extern "C" int exacto_rccl_comm_destroy(void* comm) {
    if (!comm) return 0;
    if (int e = rccl_ready()) return e;
    {
        std::lock_guard<std::mutex> g(g_aborted_mu);
        if (g_aborted.erase(comm)) return 0;   // freed by ncclCommAbort
    }
    RCCL_TRY(rccl().comm_destroy((ncclComm_t)comm));
    return 0;
}

extern "C" int exacto_rccl_sync(exacto_ctx* c, void* comm) {
    if (int e = check_ctx(c)) return e;
    if (!comm) return invalid_param("null communicator");
    if (int e = rccl_ready()) return e;
    return rccl_stream_wait(c, comm, "collective on the context stream");
}

extern "C" int exacto_rccl_comm_count(void* comm, int* nranks) {
    if (!comm || !nranks) return invalid_param("null argument");
    if (int e = rccl_ready()) return e;
    RCCL_TRY(rccl().comm_count((ncclComm_t)comm, nranks));
    return 0;
}

// In-place broadcast of `words` u64 at buf from root's buffer, enqueued on the context stream.
// Checks the communicator and the root first; *my_rank (optional) receives this rank.
static int rccl_check(void* comm, int root, int* my_rank) {
    if (!comm) return invalid_param("null communicator");
    if (int e = rccl_ready()) return e;
    int nr = 0;
    RCCL_TRY(rccl().comm_count((ncclComm_t)comm, &nr));
    if (root < 0 || root >= nr) return invalid_param("root out of range");
    if (my_rank) RCCL_TRY(rccl().comm_user_rank((ncclComm_t)comm, my_rank));
    return 0;
}

static int rccl_bcast(exacto_ctx* c, void* comm, int root, u64* buf, size_t words) {
    if (int e = rccl_check(comm, root, nullptr)) return e;
    if (!words) return 0;
    RCCL_TRY(rccl().broadcast(buf, buf, words, ncclUint64, root, (ncclComm_t)comm, c->stream));
    return 0;
}

// Agreement step of a collective call: every rank contributes {its num_keys, its own verdict} and
// all-gathers everyone's, so that every rank takes the same decision (proceed or InvalidParam)
// before any rank resizes its key or enqueues the key broadcast.  A mismatch therefore fails on all
// ranks instead of leaving the others blocked in a broadcast the failing rank never joins.
static int rccl_agree(exacto_ctx* c, void* comm, u64 mine, u64 ok, bool* agreed, std::string* why) {
    *agreed = false;
    int nr = 0;
    RCCL_TRY(rccl().comm_count((ncclComm_t)comm, &nr));
    DevBuf<u64> dev;
    if (int e = dev.alloc(sizeof(u64) * 2 * (nr + 1))) return e;
    std::vector<u64> host(2 * (size_t)(nr + 1));
    host[0] = mine;
    host[1] = ok;
    int rc = 0;
    if (hipMemcpyAsync(dev, host.data(), 2 * sizeof(u64), hipMemcpyHostToDevice, c->stream) != hipSuccess)
        rc = fail(EXACTO_ERR_HIP, "HIP error: hipMemcpyAsync (agreement header)");
    else {
        const ncclResult_t r = rccl().all_gather(dev, dev + 2, 2, ncclUint64, (ncclComm_t)comm, c->stream);
        if (r != ncclSuccess)
            rc = fail(EXACTO_ERR_HIP, std::string("RCCL error: ") + rccl().error_string(r) + " (ncclAllGather)");
        else if (hipMemcpyAsync(host.data() + 2, dev + 2, 2 * sizeof(u64) * nr, hipMemcpyDeviceToHost, c->stream) !=
                     hipSuccess ||
                 (rc = rccl_stream_wait(c, comm, "agreement all-gather")) != 0) {
            if (!rc) rc = fail(EXACTO_ERR_HIP, "HIP error: agreement header read-back");
        }
    }
    if (rc) {   // a timed-out all-gather may still own `dev`, and a release would wait for it: leave the
                // block to a holder that is never destroyed (the process is ending)
        (void)new DevBuf<u64>(std::move(dev));
        return rc;
    }
    (void)hipStreamSynchronize(c->stream);
    for (int r = 0; r < nr; ++r) {
        if (!host[2 + 2 * r + 1]) {
            *why = "rank " + std::to_string(r) + " rejected the call";
            return 0;
        }
        if (host[2 + 2 * r] != host[2]) {
            *why = "ranks disagree on num_keys (rank 0: " + std::to_string(host[2]) + ", rank " + std::to_string(r) +
                   ": " + std::to_string(host[2 + 2 * r]) + ")";
            return 0;
        }
    }
    *agreed = true;
    return 0;
}

// Every check runs before the resident key is touched: a failed call (bad root, no RCCL, a root
// without a loaded key of that size, ranks passing different num_keys) leaves every rank's key
// exactly as it was and returns InvalidParam on every rank (rccl_agree).  The root broadcasts its
// resident key as loaded (never resized); a receiving rank's buffer is (re)sized and marked loaded
// only once the broadcast into it has been enqueued.
extern "C" int exacto_ctx_broadcast_relin_key(exacto_ctx* c, void* comm, int root, size_t num_keys) {
    if (int e = check_ctx(c)) return e;
    int me = -1;
    if (int e = rccl_check(comm, root, &me)) return e;
    const size_t words = num_keys * 2 * c->L * (size_t)c->n;
    const bool root_ok = c->rlk_loaded && c->rlk_keys == num_keys;
    std::string why;
    bool agreed = false;
    if (int e = rccl_agree(c, comm, num_keys, me == root ? root_ok : 1, &agreed, &why)) return e;
    if (!agreed) {
        if (me == root && !root_ok)
            why = "broadcast root has no resident relinearization key of " + std::to_string(num_keys) + " rows";
        return invalid_param(why);
    }
    if (me == root) {
        if (!words) return 0;
        RCCL_TRY(rccl().broadcast(c->d_rlk, c->d_rlk, words, ncclUint64, root, (ncclComm_t)comm, c->stream));
        return 0;
    }
    u64* dst = exacto_ctx_relin_key_buffer(c, num_keys);
    if (!dst) return fail(EXACTO_ERR_HIP, "HIP error: relinearization key allocation failed");
    if (words) {
        const ncclResult_t r = rccl().broadcast(dst, dst, words, ncclUint64, root, (ncclComm_t)comm, c->stream);
        if (r != ncclSuccess) {
            c->rlk_loaded = false;   // the buffer's contents are undefined now
            return fail(EXACTO_ERR_HIP, std::string("RCCL error: ") + rccl().error_string(r) + " (ncclBroadcast)");
        }
    }
    return 0;
}

extern "C" int exacto_broadcast_galois_key(exacto_ctx* c, void* comm, int root, uint64_t* gk, size_t num_keys) {
    if (int e = check_ctx(c)) return e;
    if (num_keys && !gk) return invalid_param("null Galois key");
    return rccl_bcast(c, comm, root, gk, num_keys * 2 * c->L * (size_t)c->n);
}

extern "C" int exacto_rccl_allgather_u64(exacto_ctx* c, void* comm, const uint64_t* send, uint64_t* recv, size_t count) {
    if (int e = check_ctx(c)) return e;
    if (!comm) return invalid_param("null communicator");
    if (count && (!send || !recv)) return invalid_param("null buffer");
    if (int e = rccl_ready()) return e;
    if (!count) return 0;
    RCCL_TRY(rccl().all_gather(send, recv, count, ncclUint64, (ncclComm_t)comm, c->stream));
    return 0;
}
