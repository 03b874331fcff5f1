// wk_api_comm.cpp -- the multi-GPU gradient exchange: which contexts it refuses, the RCCL
// communicator, the host all-reduce callback, the IPC region over peer-mapped memory and its
// status, the exchange leg of a minibatch, and the record exchange (wk_comm_records): the gather of
// the ranks' statistics records and its header check.  The only host unit that sees rccl.h.
#include <rccl/rccl.h>

#include <cstdlib>
#include <cstring>

#include "wk_ctx.h"
#include "wk_text.h"

// records: the initialiser serves the record exchange and the context declared it
// (wk_comm_records), so every rank decides on the ranks' summed statistics
static int refuse_comm(wk_ctx* c, bool records = false) {
  if (records && c->rx_kind != wk_ctx::RX_NONE) return WK_OK;  // (never a general context)
  // ranks scaling their rewards by their own shards' statistics would train on different targets
  if (c->rn_on) {
    SETERR(c, "the multi-GPU gradient exchange refuses a context with reward normalisation enabled: "
              "every rank would scale by its own shard's statistics");
    return WK_ERR_CONFIG;
  }
  // ranks that stop on their own shards' KL would desert each other mid-exchange
  if (c->cfg.TargetKL > 0.0f) {
    SETERR(c, "the multi-GPU gradient exchange refuses a TargetKL > 0 context: every rank would "
              "decide on its own shard's statistics");
    return WK_ERR_CONFIG;
  }
  // ranks stepping the log-std on their own shards' gradients would diverge
  if (c->cfg.LearnLogStd == 1) {
    SETERR(c, "the multi-GPU gradient exchange refuses a LearnLogStd = 1 context: every rank would "
              "step the log-std on its own shard's gradient");
    return WK_ERR_CONFIG;
  }
  if (!c->general) return WK_OK;
  SETERR(c, "the multi-GPU gradient exchange serves the built-in kernels only (NetworkKernels = 0)");
  return WK_ERR_CONFIG;
}

// the IPC exchange applies Adam inside the launch that sums the ranks: no launch boundary at
// which the norm of the summed gradient could be formed
static int refuse_ipc_clip(wk_ctx* c) {
  if (!c->gnorm) return WK_OK;
  SETERR(c, "the IPC gradient exchange refuses a MaxGradNorm > 0 context: it fuses reduction, exchange "
            "and Adam in one launch (wk_comm_init and wk_comm_init_host clip the summed gradient)");
  return WK_ERR_CONFIG;
}

// the ring slot of the next stamped exchange launch (wk_comm_xch_profile), or null
uint64_t* xch_stamp_slot(wk_ctx* c) {
  if (!c->xch_stamps) return nullptr;
  const int64_t slot = c->xch_stamp_launches++ % c->xch_stamp_cap;
  return c->xch_stamps + (size_t)slot * wk::xch_blocks() * wk::XCH_POINTS;
}

// IPC contexts: WK_ERR_COMM once an exchange timed out or met a peer's abort (from then on every
// exchange is a no-op); the host's Adam step count rolls back to the last step block 0 applied
// (wk_get_adam and checkpoints report the steps actually taken)
int xch_status(wk_ctx* c) {
  if (!c->ipc) return WK_OK;
  uint32_t err[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(err, c->xch_err, sizeof err, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (err[0]) {
    c->adam_t = (int)err[1];
    SETERR(c, "IPC gradient exchange: a peer did not publish its minibatch slab within %.1f s or "
           "gave up on it (no Adam step applied since step %u; the replicas may differ and this "
           "context stays failed: stop the job, or on every rank destroy the context, create and "
           "map a new one and load a checkpoint)",
           (double)c->xch_timeout_ticks / wk::XCH_TICKS_PER_S, err[1]);
    return WK_ERR_COMM;
  }
  return WK_OK;
}

// the device's record of the last applied Adam step starts from the host's count (a checkpoint
// or wk_set_adam may have moved it since the last exchange)
int xch_mark_t(wk_ctx* c) {
  if (!c->ipc) return WK_OK;
  HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(c->xch_err + 1), (int)c->adam_t, 1, c->stream));
  return WK_OK;
}

static uint64_t xch_ticks_of(double seconds) {
  return (uint64_t)(seconds * wk::XCH_TICKS_PER_S);
}

int wk_comm_set_timeout(wk_ctx* c, double seconds) {
  if (!c || !(seconds > 0.0) || seconds > 1.0e6) return WK_ERR_ARG;
  c->xch_timeout_ticks = xch_ticks_of(seconds);
  return WK_OK;
}

// The exchange leg of a minibatch, between the block reduction and Adam (RCCL and host contexts;
// the IPC exchange has all three in one launch): the summed slab in c->grad over the ranks
int comm_exchange(wk_ctx* c) {
  ProfScope ps(c, PK_ALLRED, 0, 2);
  if (c->comm) {
    ncclResult_t r = ncclAllReduce(c->grad, c->grad, wk::SLAB, ncclFloat, ncclSum,
                                   c->comm, c->stream);
    if (r != ncclSuccess) { SETERR(c, "ncclAllReduce: %s", ncclGetErrorString(r)); return WK_ERR_COMM; }
  } else {  // host all-reduce: the slab goes through the caller's function between two copies
    c->host_ar_buf.resize(wk::SLAB);
    HIPCHK(c, hipMemcpyAsync(c->host_ar_buf.data(), c->grad, sizeof(float) * wk::SLAB,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->host_ar(c->host_ar_buf.data(), wk::SLAB, c->host_ar_user) != 0) {
      SETERR(c, "host all-reduce callback failed");
      return WK_ERR_COMM;
    }
    HIPCHK(c, hipMemcpyAsync(c->grad, c->host_ar_buf.data(), sizeof(float) * wk::SLAB,
                             hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host buffer is reused next minibatch
  }
  return WK_OK;
}

// wk_destroy: the communicator, the peers' mappings and this rank's region
void comm_close(wk_ctx* c) {
  if (c->comm) ncclCommDestroy(c->comm);
  for (void* p : c->xch_peers)
    if (p) (void)hipIpcCloseMemHandle(p);
  if (c->xch) (void)hipFree(c->xch);
}

// ---------------- the record exchange ----------------
static_assert(WK_COMM_RECORD_WORDS == wk::RECORD_WORDS, "record width");

int wk_comm_records(wk_ctx* c, wk_host_allgather_fn* fn, void* user) {
  if (!c) return WK_ERR_ARG;
  if (c->general) {
    SETERR(c, "wk_comm_records: the record exchange serves the built-in kernels only (NetworkKernels = 0)");
    return WK_ERR_CONFIG;
  }
  if (c->comm || c->host_ar || c->ipc || c->xch) {
    SETERR(c, "wk_comm_records comes before the gradient exchange is initialised");
    return WK_ERR_STATE;
  }
  if (c->rx_kind != wk_ctx::RX_NONE) { SETERR(c, "wk_comm_records was already called on this context"); return WK_ERR_STATE; }
  c->rx_kind = fn ? wk_ctx::RX_HOST : wk_ctx::RX_RCCL;
  c->rx_fn = fn;
  c->rx_user = user;
  return WK_OK;
}

// the initialiser `kind` against the declared record exchange
static int rx_match(wk_ctx* c, int kind) {
  if (c->rx_kind == wk_ctx::RX_NONE || c->rx_kind == kind) return WK_OK;
  SETERR(c, "wk_comm_records declared %s: initialise the gradient exchange with %s",
         c->rx_kind == wk_ctx::RX_RCCL ? "the RCCL record exchange" : "a host record exchange",
         c->rx_kind == wk_ctx::RX_RCCL ? "wk_comm_init" : "wk_comm_init_host");
  return WK_ERR_STATE;
}

// the gather buffer and the error word, once the number of ranks is known
static int rx_alloc(wk_ctx* c, int nranks) {
  if (c->rx_kind == wk_ctx::RX_NONE) return WK_OK;
  const size_t bytes = sizeof(uint64_t) * wk::RECORD_WORDS * (size_t)nranks;
  HIPCHK(c, dev_alloc(c, &c->rx_dev, bytes));
  HIPCHK(c, hipMemset(c->rx_dev, 0, bytes));
  HIPCHK(c, dev_alloc(c, &c->rx_err, sizeof(uint32_t)));
  HIPCHK(c, hipMemset(c->rx_err, 0, sizeof(uint32_t)));
  c->rx_host.assign((size_t)wk::RECORD_WORDS * nranks, 0);
  return WK_OK;
}

uint64_t rx_header(wk_ctx* c, int kind) {
  const uint64_t seq = c->rx_seq++ & ((1ull << 48) - 1);
  return ((uint64_t)kind << 56) | ((uint64_t)(c->nranks & 0xff) << 48) | seq;
}

static int rx_fail(wk_ctx* c, int rank, uint64_t got, uint64_t want) {
  SETERR(c, "record exchange: rank %d's record has header %016llx where this rank (%d) has %016llx "
            "(kind << 56 | nranks << 48 | sequence): the ranks' calls are out of step -- fatal for the "
            "job, abort every rank", rank, (unsigned long long)got, c->rank, (unsigned long long)want);
  return WK_ERR_COMM;
}

// every gathered header against this rank's own
static int rx_check(wk_ctx* c, uint64_t header) {
  for (int r = 0; r < c->nranks; r++) {
    const uint64_t h = c->rx_host[(size_t)r * wk::RECORD_WORDS];
    if (h != header) return rx_fail(c, r, h, header);
  }
  return WK_OK;
}

int rx_deferred(wk_ctx* c) {
  if (!c->rx_pending) return WK_OK;
  uint32_t err = 0;
  HIPCHK(c, hipMemcpyAsync(&err, c->rx_err, sizeof err, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->rx_pending = false;
  if (!err) return WK_OK;
  SETERR(c, "record exchange (reward normalisation): rank %u's record carried another header than this "
            "rank's (%d): the ranks' calls are out of step, nothing was merged -- fatal for the job, "
            "abort every rank", err - 1u, c->rank);
  return WK_ERR_COMM;
}

// the host control plane: this rank's slot out, the caller's all-gather, the headers checked
static int rx_host_round(wk_ctx* c, uint64_t header) {
  uint64_t mine[wk::RECORD_WORDS];
  HIPCHK(c, hipMemcpyAsync(mine, c->rx_dev + (size_t)c->rank * wk::RECORD_WORDS, sizeof mine,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::fill(c->rx_host.begin(), c->rx_host.end(), 0);
  if (c->rx_fn(mine, c->rx_host.data(), c->rx_user) != 0) {
    SETERR(c, "host record all-gather callback failed");
    return WK_ERR_COMM;
  }
  return rx_check(c, header);
}

static int rx_nccl_gather(wk_ctx* c) {
  ncclResult_t r = ncclAllGather(c->rx_dev + (size_t)c->rank * wk::RECORD_WORDS, c->rx_dev,
                                 wk::RECORD_WORDS, ncclUint64, c->comm, c->stream);
  if (r != ncclSuccess) { SETERR(c, "ncclAllGather: %s", ncclGetErrorString(r)); return WK_ERR_COMM; }
  return WK_OK;
}

int rx_gather_device(wk_ctx* c, uint64_t header) {
  if (c->comm) {  // stream-ordered: the consumer kernel checks the headers (rx_deferred reports)
    if (int r = rx_nccl_gather(c)) return r;
    c->rx_pending = true;
    return WK_OK;
  }
  if (int r = rx_host_round(c, header)) return r;
  HIPCHK(c, hipMemcpyAsync(c->rx_dev, c->rx_host.data(), sizeof(uint64_t) * c->rx_host.size(),
                           hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the host buffer is reused by the next exchange
  return WK_OK;
}

int rx_gather_host(wk_ctx* c, uint64_t header) {
  if (!c->comm) return rx_host_round(c, header);
  if (int r = rx_nccl_gather(c)) return r;
  HIPCHK(c, hipMemcpyAsync(c->rx_host.data(), c->rx_dev, sizeof(uint64_t) * c->rx_host.size(),
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return rx_check(c, header);
}

int wk_comm_unique_id(uint8_t* id) {
  if (!id) return WK_ERR_ARG;
  static_assert(sizeof(ncclUniqueId) == 128, "nccl id size");
  ncclUniqueId u;
  ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess) { wk::set_last_error(ncclGetErrorString(r)); return WK_ERR_COMM; }
  memcpy(id, &u, sizeof(u));
  return WK_OK;
}

int wk_comm_init(wk_ctx* c, int rank, int nranks, const uint8_t* id) {
  DevGuard dg_(c);
  if (!c || !id || nranks <= 0 || rank < 0 || rank >= nranks) return WK_ERR_ARG;
  if (int r = rx_match(c, wk_ctx::RX_RCCL)) return r;
  if (int r = refuse_comm(c, true)) return r;
  if (c->rx_kind && nranks > 255) { SETERR(c, "the record exchange spans at most 255 ranks"); return WK_ERR_ARG; }
  if (c->host_ar) { SETERR(c, "the context already has a host all-reduce"); return WK_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  ncclResult_t r = ncclCommInitRank(&c->comm, nranks, u, rank);
  if (r != ncclSuccess) { SETERR(c, "ncclCommInitRank: %s", ncclGetErrorString(r)); c->comm = nullptr; return WK_ERR_COMM; }
  c->rank = rank;
  c->nranks = nranks;
  return rx_alloc(c, nranks);
}

int wk_comm_init_host(wk_ctx* c, int rank, int nranks, wk_host_allreduce_fn fn, void* user) {
  DevGuard dg_(c);
  if (!c || !fn || nranks <= 0 || rank < 0 || rank >= nranks) return WK_ERR_ARG;
  if (int r = rx_match(c, wk_ctx::RX_HOST)) return r;
  if (int r = refuse_comm(c, true)) return r;
  if (c->rx_kind && nranks > 255) { SETERR(c, "the record exchange spans at most 255 ranks"); return WK_ERR_ARG; }
  if (c->comm) { SETERR(c, "the context already has an RCCL communicator"); return WK_ERR_STATE; }
  if (int r = rx_alloc(c, nranks)) return r;
  c->host_ar = fn;
  c->host_ar_user = user;
  c->rank = rank;
  c->nranks = nranks;
  return WK_OK;
}

// the exchange record of one rank: [0, 64) the region's hipIpcMemHandle_t, [64, 128) the PCI bus
// id of the rank's device (NUL-padded), so every rank can count the ranks sharing its GPU
static constexpr size_t kIpcDevOff = 64;
static_assert(sizeof(hipIpcMemHandle_t) == kIpcDevOff && WK_IPC_HANDLE_BYTES == 128, "IPC record");

int wk_comm_ipc_handle(wk_ctx* c, uint8_t* handle) {
  DevGuard dg_(c);
  if (!c || !handle) return WK_ERR_ARG;
  if (int r = refuse_comm(c)) return r;
  if (int r = refuse_ipc_clip(c)) return r;
  if (int r = rx_match(c, -1)) return r;  // (the IPC exchange carries no records)
  if (!c->xch) {
    // uncached (MTYPE UC) device memory: the peers read it over xGMI and this GPU writes it
    // through no cache; coarse-grained hipMalloc memory is the fallback where the driver cannot
    // export an uncached allocation (the system-scope release / acquire covers it as well)
    const size_t bytes = wk::xch_region_bytes();
    hipIpcMemHandle_t probe;
    if (hipExtMallocWithFlags(&c->xch, bytes, hipDeviceMallocUncached) != hipSuccess ||
        hipIpcGetMemHandle(&probe, c->xch) != hipSuccess) {
      if (c->xch) (void)hipFree(c->xch);
      c->xch = nullptr;
      (void)hipGetLastError();
      HIPCHK(c, hipMalloc(&c->xch, bytes));
      c->xch_uncached = false;
    } else {
      c->xch_uncached = true;
    }
    HIPCHK(c, hipMemset(c->xch, 0, bytes));
    HIPCHK(c, dev_alloc(c, &c->xch_err, 2 * sizeof(uint32_t)));
    HIPCHK(c, hipMemset(c->xch_err, 0, 2 * sizeof(uint32_t)));
  }
  hipIpcMemHandle_t h;
  HIPCHK(c, hipIpcGetMemHandle(&h, c->xch));
  memset(handle, 0, WK_IPC_HANDLE_BYTES);
  memcpy(handle, &h, sizeof h);
  HIPCHK(c, hipDeviceGetPCIBusId((char*)handle + kIpcDevOff, (int)(WK_IPC_HANDLE_BYTES - kIpcDevOff) - 1,
                                 c->device));
  return WK_OK;
}

int wk_comm_init_ipc(wk_ctx* c, int rank, int nranks, const uint8_t* handles) {
  DevGuard dg_(c);
  if (!c || !handles || nranks <= 0 || rank < 0 || rank >= nranks) return WK_ERR_ARG;
  if (int r = refuse_comm(c)) return r;
  if (int r = refuse_ipc_clip(c)) return r;
  if (int r = rx_match(c, -1)) return r;  // (the IPC exchange carries no records)
  if (nranks > wk::XCH_MAX_RANKS) { SETERR(c, "the IPC exchange spans at most %d ranks", (int)wk::XCH_MAX_RANKS); return WK_ERR_ARG; }
  if (c->comm || c->host_ar || c->ipc) { SETERR(c, "the context already has an all-reduce"); return WK_ERR_STATE; }
  if (!c->xch) { SETERR(c, "wk_comm_ipc_handle first"); return WK_ERR_STATE; }
  {  // ranks sharing this rank's GPU (a rehearsal): more than four stall, see XCH_MAX_RANKS_PER_DEVICE
    const char* mine = (const char*)handles + (size_t)rank * WK_IPC_HANDLE_BYTES + kIpcDevOff;
    int same = 0;
    for (int r = 0; r < nranks; r++)
      same += strncmp(mine, (const char*)handles + (size_t)r * WK_IPC_HANDLE_BYTES + kIpcDevOff,
                      WK_IPC_HANDLE_BYTES - kIpcDevOff) == 0;
    if (same > wk::XCH_MAX_RANKS_PER_DEVICE) {
      SETERR(c, "the IPC exchange takes at most %d ranks per GPU (%d share %s): their waiting "
             "exchange blocks would hold the CUs a peer's gradient kernel needs",
             (int)wk::XCH_MAX_RANKS_PER_DEVICE, same, mine);
      return WK_ERR_ARG;
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  wk::XchArgs x{};
  std::vector<void*> opened;
  for (int r = 0; r < nranks; r++) {
    void* base = c->xch;
    if (r != rank) {
      hipIpcMemHandle_t h;
      memcpy(&h, handles + (size_t)r * WK_IPC_HANDLE_BYTES, sizeof h);
      const hipError_t e = hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess);
      if (e != hipSuccess) {
        for (void* p : opened) (void)hipIpcCloseMemHandle(p);
        SETERR(c, "hipIpcOpenMemHandle (rank %d): %s", r, hipGetErrorString(e));
        return WK_ERR_COMM;
      }
      opened.push_back(base);
    }
    x.slab[r] = (float*)base;
    x.flag[r] = (uint64_t*)((char*)base + sizeof(float) * 2 * wk::SLAB);
  }
  x.rank = rank;
  x.nranks = nranks;
  c->xa = x;
  if (c->xch_timeout_ticks == 0) {  // wk_comm_set_timeout before the mapping wins
    double sec = wk::XCH_TIMEOUT_S_DEFAULT;
    if (const char* e = getenv("WK_XCH_TIMEOUT_S")) {
      const double v = atof(e);
      if (v > 0.0 && v <= 1.0e6) sec = v;
    }
    c->xch_timeout_ticks = xch_ticks_of(sec);
  }
  c->xch_peers = opened;
  c->ipc = true;
  c->rank = rank;
  c->nranks = nranks;
  return WK_OK;
}

int wk_comm_info(wk_ctx* c, int* kind, int* flags) {
  if (!c || !kind || !flags) return WK_ERR_ARG;
  *kind = c->ipc ? 3 : c->host_ar ? 2 : c->comm ? 1 : 0;
  *flags = (c->xch && c->xch_uncached) ? 1 : 0;
  return WK_OK;
}

int wk_comm_xch_profile(wk_ctx* c, int minibatches) {
  DevGuard dg_(c);
  if (!c || minibatches < 0 || minibatches > (1 << 20)) return WK_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (no launch still writes the old ring)
  if (c->xch_stamps) (void)hipFree(c->xch_stamps);
  c->xch_stamps = nullptr;
  c->xch_stamp_cap = 0;
  c->xch_stamp_launches = 0;
  if (minibatches == 0) return WK_OK;
  const size_t bytes = sizeof(uint64_t) * (size_t)minibatches * wk::xch_blocks() * wk::XCH_POINTS;
  HIPCHK(c, dev_alloc(c, &c->xch_stamps, bytes));
  HIPCHK(c, hipMemset(c->xch_stamps, 0, bytes));
  c->xch_stamp_cap = minibatches;
  return WK_OK;
}

int wk_comm_xch_stamps(wk_ctx* c, uint64_t* stamps, int max_launches, int* launches, int* blocks) {
  DevGuard dg_(c);
  if (!c || !launches || !blocks || max_launches < 0 || (max_launches > 0 && !stamps)) return WK_ERR_ARG;
  *blocks = wk::xch_blocks();
  if (!c->xch_stamps) { *launches = 0; return WK_OK; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t have = std::min<int64_t>(c->xch_stamp_launches, c->xch_stamp_cap);
  const int n = (int)std::min<int64_t>(have, max_launches);
  const size_t per = (size_t)wk::xch_blocks() * wk::XCH_POINTS;
  // the last n launches, oldest first (the ring wraps at cap)
  for (int i = 0; i < n; i++) {
    const int64_t launch = c->xch_stamp_launches - n + i;
    const int64_t slot = launch % c->xch_stamp_cap;
    HIPCHK(c, hipMemcpy(stamps + (size_t)i * per, c->xch_stamps + (size_t)slot * per,
                        sizeof(uint64_t) * per, hipMemcpyDeviceToHost));
  }
  *launches = n;
  return WK_OK;
}

int wk_allreduce_test(wk_ctx* c, float* host_buf, int n) {
  DevGuard dg_(c);
  if (!c || !host_buf || n <= 0) return WK_ERR_ARG;
  if (c->ipc) {  // one round of the IPC exchange (k_reduce_xch_adam without Adam) on this slab
    if (n > wk::SLAB) { SETERR(c, "the IPC exchange test takes at most %d floats", (int)wk::SLAB); return WK_ERR_ARG; }
    if (ensure(c, &c->scratch, &c->scratch_bytes, sizeof(float) * 2 * wk::SLAB)) return WK_ERR_HIP;
    float* in = (float*)c->scratch;
    float* out = in + wk::SLAB;
    HIPCHK(c, hipMemsetAsync(in, 0, sizeof(float) * wk::SLAB, c->stream));
    HIPCHK(c, hipMemcpyAsync(in, host_buf, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    wk::XchArgs x = c->xa;
    x.partial = in;
    x.nblocks = 1;
    x.grad_out = out;
    x.seq = ++c->xch_seq;
    x.err = c->xch_err;
    x.timeout_ticks = c->xch_timeout_ticks;
    x.a = wk::AdamArgs{};
    HIPCHK(c, wk::launch_reduce_xch_adam(x, c->stream));
    HIPCHK(c, hipMemcpyAsync(host_buf, out, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return xch_status(c);
  }
  if (ensure(c, &c->scratch, &c->scratch_bytes, sizeof(float) * n)) return WK_ERR_HIP;
  HIPCHK(c, hipMemcpyAsync(c->scratch, host_buf, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
  if (c->comm && c->nranks > 1) {
    ncclResult_t r = ncclAllReduce(c->scratch, c->scratch, n, ncclFloat, ncclSum, c->comm, c->stream);
    if (r != ncclSuccess) { SETERR(c, "ncclAllReduce: %s", ncclGetErrorString(r)); return WK_ERR_COMM; }
  }
  HIPCHK(c, hipMemcpyAsync(host_buf, c->scratch, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return WK_OK;
}
