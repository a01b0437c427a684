// scfq_scratch.hip — the library-owned scratch of the record pipelines (scfq_scratch.hpp): one memory pool per device, the
// idle streams, the caller-stream rule, and their release at shutdown.
#include "scfq_scratch.hpp"

#include <map>
#include <mutex>
#include <vector>

namespace {

// Scratch comes from a stream-ordered memory pool OWNED BY THIS LIBRARY (one per device, release threshold = keep
// everything, destroyed by scfq_shutdown): after the first call a record pipeline allocates nothing from the driver
// (hipMalloc / hipFree of multi-GB buffers cost more than all kernels of fq-dedup together), and the device's default
// pool — which belongs to the host application — is left as it was.
std::mutex g_pool_mu;
std::map<int, hipMemPool_t> g_pools;

// The call's private stream comes from a per-device list of idle ones and goes back to it (r4: creating and destroying a stream per
// call cost more host time than all the launches of the pipeline; scfq_shutdown destroys them).  A stream is only returned by a call
// that has waited for everything it put on it.
std::map<int, std::vector<hipStream_t>> g_idle_streams;      // under g_pool_mu

}  // namespace

namespace scfq_scratch {

int pool(hipMemPool_t* out, char* errbuf) {
  int dev = 0;
  SCFQ_SCRATCH_CHK(errbuf, hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_pool_mu);
  auto it = g_pools.find(dev);
  if (it == g_pools.end()) {
    hipMemPoolProps props{};
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    hipMemPool_t mp = nullptr;
    SCFQ_SCRATCH_CHK(errbuf, hipMemPoolCreate(&mp, &props));
    uint64_t keep = UINT64_MAX;
    SCFQ_SCRATCH_CHK(errbuf, hipMemPoolSetAttribute(mp, hipMemPoolAttrReleaseThreshold, &keep));
    it = g_pools.emplace(dev, mp).first;
  }
  *out = it->second;
  return SCFQ_OK;
}

int lease_stream(hipStream_t* s, int* dev, char* errbuf) {
  SCFQ_SCRATCH_CHK(errbuf, hipGetDevice(dev));
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto& v = g_idle_streams[*dev];
    if (!v.empty()) { *s = v.back(); v.pop_back(); return SCFQ_OK; }
  }
  SCFQ_SCRATCH_CHK(errbuf, hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  return SCFQ_OK;
}

void return_stream(hipStream_t s, int dev, bool clean) {
  if (clean || hipStreamSynchronize(s) == hipSuccess) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto& v = g_idle_streams[dev];
    if (v.size() < 8) { v.push_back(s); return; }
  }
  (void)hipStreamDestroy(s);
}

int order_after_caller(hipStream_t stream, char* errbuf) {
  int on = 0;
  void* ws = scfq_get_wait_stream(&on);
  if (!on) return SCFQ_OK;
  hipEvent_t ev;
  SCFQ_SCRATCH_CHK(errbuf, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, static_cast<hipStream_t>(ws));
  if (e == hipSuccess) e = hipStreamWaitEvent(stream, ev, 0);
  (void)hipEventDestroy(ev);
  SCFQ_SCRATCH_CHK(errbuf, e);
  return SCFQ_OK;
}

void release_all() {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (auto& kv : g_idle_streams) { if (hipSetDevice(kv.first) == hipSuccess) for (hipStream_t st : kv.second) (void)hipStreamDestroy(st); }
  g_idle_streams.clear();
  for (auto& kv : g_pools) { if (hipSetDevice(kv.first) == hipSuccess) (void)hipMemPoolDestroy(kv.second); }
  g_pools.clear();
}

}  // namespace scfq_scratch
