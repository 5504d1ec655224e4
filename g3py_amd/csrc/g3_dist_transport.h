// Transports of the multi-GPU driver (g3_dist.hip): how a rank's collectives reach its peers.  RCCL (the product; dlopen,
// so a single-GPU user never needs librccl) or caller-supplied host callbacks (tests: several ranks sharing ONE GPU over
// gloo -- RCCL refuses two ranks on one device -- so the schedule is checked for P > 1 on a one-GPU box), blocking or
// served by worker threads.  The replay transport needs the driver object and lives with it.  Included by g3_dist.hip only.
#pragma once
#include "g3_internal.h"
#include "g3_host.h"

#include <dlfcn.h>
#include <rccl/rccl.h>
#include <stdlib.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

namespace {

enum { G3_COLL_BCAST = 0, G3_COLL_ALLGATHER = 1, G3_COLL_ALLREDUCE = 2, G3_NCOLL = 3, G3_PH_DIAG = 3, G3_PH_SOLVE = 4, G3_NKIND = 5 };

struct Transport {
  virtual ~Transport() {}
  // stream-ordered after everything queued on s; the result is visible to work queued on s afterwards
  virtual int bcast(void* buf, size_t bytes, int root, hipStream_t s) = 0;
  virtual int allgather(const void* send, void* recv, size_t bytes_per_rank, hipStream_t s) = 0;
  // host values in / out; synchronises s.  op: 0 sum, 1 min, 2 max
  virtual int allreduce(double* host, int n, int op, hipStream_t s) = 0;
  virtual const char* name() const = 0;
  // what the NEXT collective carries (G3_HINT_*, index of the block / panel): only the replay transport needs to know
  virtual void hint(int what, int index) { (void)what; (void)index; }
  char err[256] = {0};
};
enum { G3_HINT_NONE = 0, G3_HINT_DIAG = 1, G3_HINT_PANEL = 2, G3_HINT_AVEC = 3 };

struct RcclApi {
  void* h = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommAbort) CommAbort = nullptr;      // optional
  decltype(&ncclBroadcast) Broadcast = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
};

static RcclApi* rccl_api(char* err, size_t errlen) {
  static RcclApi api;
  static int state = 0;   // 0 untried, 1 ok, -1 failed
  if (state == 1) return &api;
  if (state == -1) return nullptr;
  // a copy already loaded into the process (e.g. the one PyTorch ships) is reused; G3_RCCL_PATH overrides
  const char* forced = getenv("G3_RCCL_PATH");
  const bool only = forced && *forced;          // a path given explicitly is the ONLY candidate: a wrong one fails loudly
  const char* names[] = {forced, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (int pass = 0; pass < 2 && !api.h; ++pass)
    for (const char* n : names) {
      if (!n || !*n) continue;
      if (only && n != forced) break;
      api.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL | (pass == 0 ? RTLD_NOLOAD : 0));
      if (api.h) break;
    }
  if (!api.h) {
    snprintf(err, errlen, "librccl not found (set G3_RCCL_PATH): %s", dlerror());
    state = -1;
    return nullptr;
  }
#define G3_SYM(f)                                                        \
  api.f = (decltype(api.f))dlsym(api.h, "nccl" #f);                      \
  if (!api.f) {                                                          \
    snprintf(err, errlen, "librccl lacks nccl" #f);                      \
    state = -1;                                                          \
    return nullptr;                                                      \
  }
  G3_SYM(GetUniqueId) G3_SYM(CommInitRank) G3_SYM(CommDestroy) G3_SYM(Broadcast) G3_SYM(AllGather) G3_SYM(AllReduce)
  G3_SYM(GetErrorString)
#undef G3_SYM
  api.CommAbort = (decltype(api.CommAbort))dlsym(api.h, "ncclCommAbort");
  state = 1;
  return &api;
}

struct RcclTransport : Transport {
  RcclApi* api = nullptr;
  ncclComm_t comm_gather = nullptr;   // panel all-gathers, scalar all-reduces (chain stream)
  ncclComm_t comm_bcast = nullptr;    // diagonal-factor broadcasts (look-ahead stream): never queues behind a gather
  double* scratch = nullptr;          // device scratch of the scalar all-reduces
  double* hscratch = nullptr;         // pinned
  static const int SCR = 16384;
  bool failed = false;                // an evaluation returned an error on this rank: peers may be inside a collective
  ~RcclTransport() override {
    // after a local error the communicators are ABORTED, not destroyed: ncclCommDestroy waits for outstanding
    // collectives, which the peers of a rank that left the sweep will never complete.  (A failed rank must end the job:
    // the other ranks are by then blocked on the GPU in a collective this rank did not enter.)
    auto drop = [&](ncclComm_t c) { if (failed && api->CommAbort) api->CommAbort(c); else api->CommDestroy(c); };
    if (api && comm_gather) drop(comm_gather);
    if (api && comm_bcast) drop(comm_bcast);
    if (scratch) (void)hipFree(scratch);
    if (hscratch) (void)hipHostFree(hscratch);
  }
  int chk(ncclResult_t r, const char* what) {
    if (r == ncclSuccess) return G3_OK;
    snprintf(err, sizeof(err), "%s: %s", what, api->GetErrorString(r));
    return G3_ERR_HIP;
  }
  int bcast(void* buf, size_t bytes, int root, hipStream_t s) override {
    return chk(api->Broadcast(buf, buf, bytes, ncclChar, root, comm_bcast, s), "ncclBroadcast");
  }
  int allgather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
    return chk(api->AllGather(send, recv, bytes, ncclChar, comm_gather, s), "ncclAllGather");
  }
  int allreduce(double* host, int n, int op, hipStream_t s) override {
    for (int off = 0; off < n; off += SCR) {
      const int c = n - off < SCR ? n - off : SCR;
      memcpy(hscratch, host + off, c * sizeof(double));
      if (hipMemcpyAsync(scratch, hscratch, c * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess) return G3_ERR_HIP;
      const ncclRedOp_t o = op == 0 ? ncclSum : (op == 1 ? ncclMin : ncclMax);
      int rc = chk(api->AllReduce(scratch, scratch, c, ncclDouble, o, comm_gather, s), "ncclAllReduce");
      if (rc) return rc;
      if (hipMemcpyAsync(hscratch, scratch, c * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess) return G3_ERR_HIP;
      if (hipStreamSynchronize(s) != hipSuccess) return G3_ERR_HIP;
      memcpy(host + off, hscratch, c * sizeof(double));
    }
    return G3_OK;
  }
  const char* name() const override { return "rccl"; }
};

struct CallbackTransport : Transport {
  g3_dist_callbacks cb;
  int bcast(void* buf, size_t bytes, int root, hipStream_t s) override {
    if (hipStreamSynchronize(s) != hipSuccess) return G3_ERR_HIP;
    return cb.bcast(cb.user, buf, bytes, root) ? G3_ERR_HIP : G3_OK;
  }
  int allgather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
    if (hipStreamSynchronize(s) != hipSuccess) return G3_ERR_HIP;
    return cb.allgather(cb.user, send, recv, bytes) ? G3_ERR_HIP : G3_OK;
  }
  int allreduce(double* host, int n, int op, hipStream_t s) override {
    if (hipStreamSynchronize(s) != hipSuccess) return G3_ERR_HIP;
    return cb.allreduce(cb.user, host, n, op) ? G3_ERR_HIP : G3_OK;
  }
  const char* name() const override { return "callbacks"; }
};

// ---- asynchronous host-callback transport: the collectives as jobs of two worker threads (gather / all-reduce, and
// broadcast: the product's two communicators), stream-ordered like RCCL calls.
//   issue (host thread):  record E on the stream -> queue the job -> launch a one-wave kernel on the stream that waits for
//                         the worker's ticket (a word in pinned host memory) -> return: the host runs ahead
//   worker:               wait for E -> device -> pinned staging (its own copy stream) -> callback -> staging -> device
//                         -> publish the ticket: the stream goes on
// The wait kernel has a wall-clock limit (G3_DIST_ASYNC_TIMEOUT_S, default 120 s): a stream never hangs on a dead peer, the
// limit sets a device error word that every later transport call reports.  The workers' copy streams have NORMAL priority:
// HIP keeps separate hardware-queue pools per priority, so they never sit behind a waiting high- or low-priority stream of
// the driver.
__global__ void host_ticket_wait_kernel(const unsigned* ticket, unsigned want, unsigned long long limit, unsigned* err) {
  if (threadIdx.x != 0) return;
  const unsigned long long t0 = wall_clock64();
  unsigned spins = 0;
  while (__hip_atomic_load(ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < want) {
    __builtin_amdgcn_s_sleep(8);
    if ((++spins & 63u) == 0 && wall_clock64() - t0 > limit) {
      __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      break;
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}

struct AsyncCallbackTransport : Transport {
  g3_dist_host_callbacks cb;
  int device = 0, rank = 0, world = 1;
  struct Job {
    int kind = -1;                 // G3_COLL_*; -1: quit
    hipEvent_t ev = nullptr;
    void* buf = nullptr;           // bcast buffer / all-gather receive buffer (device)
    const void* send = nullptr;    // all-gather: this rank's part (device)
    size_t bytes = 0;
    int root = 0;
    double* vals = nullptr;        // all-reduce (host, the caller waits)
    int n = 0, op = 0;
    unsigned seq = 0;
  };
  struct Worker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv, cv_done;
    std::deque<Job> q;
    unsigned issued = 0, done = 0;       // tickets (done is mirrored in *ticket for the device)
    unsigned* ticket = nullptr;          // pinned, mapped
    unsigned* ticket_dev = nullptr;
    hipStream_t cs = nullptr;            // copy stream
    char* stage = nullptr;               // pinned staging
    size_t stage_bytes = 0;
    std::vector<char*> retired;          // outgrown staging buffers: released at teardown (hipHostFree synchronises the
                                         // DEVICE -- called while a stream waits for this worker it would never return)
    std::atomic<int> failed{0};          // set by the worker, read by the issuing thread
    char msg[200] = {0};                 // written and read under mu
  } w[2];                                // 0: all-gather + all-reduce, 1: broadcast
  unsigned* err_host = nullptr;          // pinned: a wait kernel ran into its limit
  unsigned* err_dev = nullptr;
  unsigned long long limit = 12000000000ull;
  std::vector<hipEvent_t> evpool;
  std::mutex evmu;

  int start() {
    if (hipHostMalloc((void**)&err_host, sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return G3_ERR_HIP;
    *err_host = 0;
    if (hipHostGetDevicePointer((void**)&err_dev, err_host, 0) != hipSuccess) return G3_ERR_HIP;
    const int lim = g3h_env_int("G3_DIST_ASYNC_TIMEOUT_S", 120);
    limit = (unsigned long long)(lim > 0 ? lim : 120) * 100000000ull;      // wall_clock64 ticks at 100 MHz
    for (int i = 0; i < 2; ++i) {
      if (hipHostMalloc((void**)&w[i].ticket, sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return G3_ERR_HIP;
      *w[i].ticket = 0;
      if (hipHostGetDevicePointer((void**)&w[i].ticket_dev, w[i].ticket, 0) != hipSuccess) return G3_ERR_HIP;
      if (hipStreamCreateWithFlags(&w[i].cs, hipStreamNonBlocking) != hipSuccess) return G3_ERR_HIP;
      w[i].th = std::thread([this, i]() { run(i); });
    }
    return G3_OK;
  }
  ~AsyncCallbackTransport() override {
    for (int i = 0; i < 2; ++i) {
      if (w[i].th.joinable()) {
        { std::lock_guard<std::mutex> lk(w[i].mu); w[i].q.push_back(Job()); }
        w[i].cv.notify_all();
        w[i].th.join();
      }
      if (w[i].cs) { (void)hipStreamSynchronize(w[i].cs); (void)hipStreamDestroy(w[i].cs); }
      if (w[i].stage) (void)hipHostFree(w[i].stage);
      for (char* p : w[i].retired) (void)hipHostFree(p);
      if (w[i].ticket) (void)hipHostFree(w[i].ticket);
    }
    for (hipEvent_t e : evpool) (void)hipEventDestroy(e);
    if (err_host) (void)hipHostFree(err_host);
  }
  hipEvent_t take_event() {
    std::lock_guard<std::mutex> lk(evmu);
    if (!evpool.empty()) { hipEvent_t e = evpool.back(); evpool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    return e;
  }
  void give_event(hipEvent_t e) { std::lock_guard<std::mutex> lk(evmu); evpool.push_back(e); }
  bool ensure_stage(Worker& W, size_t bytes) {
    if (W.stage_bytes >= bytes) return true;
    if (W.stage) W.retired.push_back(W.stage);       // (not freed here: see `retired`)
    W.stage = nullptr; W.stage_bytes = 0;
    bytes += bytes / 4;                              // head room: plans of one driver differ by a few blocks
    if (hipHostMalloc((void**)&W.stage, bytes, hipHostMallocDefault) != hipSuccess) return false;
    W.stage_bytes = bytes;
    return true;
  }
  void fail(Worker& W, const char* what) {
    std::lock_guard<std::mutex> lk(W.mu);
    snprintf(W.msg, sizeof(W.msg), "%s", what);
    W.failed = 1;
  }
  void run(int i) {
    Worker& W = w[i];
    (void)hipSetDevice(device);
    for (;;) {
      Job j;
      {
        std::unique_lock<std::mutex> lk(W.mu);
        W.cv.wait(lk, [&]() { return !W.q.empty(); });
        j = W.q.front();
        W.q.pop_front();
      }
      if (j.kind < 0) return;
      bool ok = !W.failed;
      if (j.ev) {
        if (hipEventSynchronize(j.ev) != hipSuccess) { ok = false; fail(W, "waiting for the stream failed"); }
        give_event(j.ev);
      }
      if (ok && j.kind == G3_COLL_BCAST) {
        ok = ensure_stage(W, j.bytes);
        if (ok && rank == j.root) ok = hipMemcpyAsync(W.stage, j.buf, j.bytes, hipMemcpyDeviceToHost, W.cs) == hipSuccess && hipStreamSynchronize(W.cs) == hipSuccess;
        if (ok) ok = cb.bcast(cb.user, W.stage, j.bytes, j.root) == 0;
        if (ok && rank != j.root) ok = hipMemcpyAsync(j.buf, W.stage, j.bytes, hipMemcpyHostToDevice, W.cs) == hipSuccess && hipStreamSynchronize(W.cs) == hipSuccess;
        if (!ok && !W.failed) fail(W, "broadcast failed (staging copy or callback)");
      } else if (ok && j.kind == G3_COLL_ALLGATHER) {
        ok = ensure_stage(W, j.bytes * (size_t)world);
        char* mine = W.stage + (size_t)rank * j.bytes;
        if (ok) ok = hipMemcpyAsync(mine, j.send, j.bytes, hipMemcpyDeviceToHost, W.cs) == hipSuccess && hipStreamSynchronize(W.cs) == hipSuccess;
        if (ok) ok = cb.allgather(cb.user, mine, W.stage, j.bytes) == 0;
        // everything but this rank's own part goes back (the in-place gather leaves that where it is; an out-of-place
        // one -- send outside the receive buffer -- gets the local copy as well)
        const bool inplace = (const char*)j.send == (const char*)j.buf + (size_t)rank * j.bytes;
        for (int q = 0; q < world && ok; ++q)
          if (q != rank || !inplace)
            ok = hipMemcpyAsync((char*)j.buf + (size_t)q * j.bytes, W.stage + (size_t)q * j.bytes, j.bytes, hipMemcpyHostToDevice, W.cs) == hipSuccess;
        if (ok) ok = hipStreamSynchronize(W.cs) == hipSuccess;
        if (!ok && !W.failed) fail(W, "all-gather failed (staging copy or callback)");
      } else if (ok && j.kind == G3_COLL_ALLREDUCE) {
        ok = cb.allreduce(cb.user, j.vals, j.n, j.op) == 0;
        if (!ok && !W.failed) fail(W, "all-reduce callback failed");
      }
      // the ticket is published even after a failure: a stream must never be left waiting (the failure is reported by
      // the next transport call and ends the evaluation with an error)
      {
        std::lock_guard<std::mutex> lk(W.mu);
        W.done = j.seq;
        __atomic_store_n(W.ticket, j.seq, __ATOMIC_RELEASE);
      }
      W.cv_done.notify_all();
    }
  }
  int check() {
    for (int i = 0; i < 2; ++i)
      if (w[i].failed) {
        std::lock_guard<std::mutex> lk(w[i].mu);
        snprintf(err, sizeof(err), "%s", w[i].msg);
        return G3_ERR_HIP;
      }
    if (*err_host) { snprintf(err, sizeof(err), "a stream waited longer than the limit for a collective (peer gone?)"); return G3_ERR_HIP; }
    return G3_OK;
  }
  int issue(int wi, Job j, hipStream_t s) {
    int rc = check();
    if (rc) return rc;
    Worker& W = w[wi];
    j.ev = take_event();
    if (!j.ev || hipEventRecord(j.ev, s) != hipSuccess) {
      if (j.ev) give_event(j.ev);
      snprintf(err, sizeof(err), "event record failed");
      return G3_ERR_HIP;
    }
    {
      std::lock_guard<std::mutex> lk(W.mu);
      j.seq = ++W.issued;
      W.q.push_back(j);
    }
    W.cv.notify_all();
    hipLaunchKernelGGL(host_ticket_wait_kernel, dim3(1), dim3(64), 0, s, (const unsigned*)W.ticket_dev, j.seq, limit, err_dev);
    if (hipGetLastError() != hipSuccess) { snprintf(err, sizeof(err), "wait-kernel launch failed"); return G3_ERR_HIP; }
    return G3_OK;
  }
  int bcast(void* buf, size_t bytes, int root, hipStream_t s) override {
    Job j; j.kind = G3_COLL_BCAST; j.buf = buf; j.bytes = bytes; j.root = root;
    return issue(1, j, s);
  }
  int allgather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
    Job j; j.kind = G3_COLL_ALLGATHER; j.send = send; j.buf = recv; j.bytes = bytes;
    return issue(0, j, s);
  }
  int allreduce(double* host, int n, int op, hipStream_t s) override {
    // behind everything queued on s and behind every gather issued so far; the caller needs the values: wait here
    Job j; j.kind = G3_COLL_ALLREDUCE; j.vals = host; j.n = n; j.op = op;
    int rc = issue(0, j, s);
    if (rc) return rc;
    Worker& W = w[0];
    unsigned want;
    { std::lock_guard<std::mutex> lk(W.mu); want = W.issued; }
    { std::unique_lock<std::mutex> lk(W.mu); W.cv_done.wait(lk, [&]() { return W.done >= want; }); }
    if (hipStreamSynchronize(s) != hipSuccess) return G3_ERR_HIP;
    return check();
  }
  const char* name() const override { return "callbacks-async"; }
};

}  // namespace
