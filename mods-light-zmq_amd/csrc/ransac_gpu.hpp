// Per-thread GPU workspace shared by the homography and the fundamental-matrix verification
// (the reference's C entry points carry no context argument, so the workspace is thread-local).
#pragma once
#include "common.hpp"
#include <mutex>
#include <sys/syscall.h>
#include <unistd.h>

namespace mods {

struct RansacGpu {
  int device = -1;
  hipStream_t stream = nullptr;
  Buf<double> u_dev;
  // hyp_cap slots: hypotheses of HYP_SLOT_BYTES on either side, and J[hyp_cap] | counts[2 * hyp_cap] in ONE allocation on either
  // side (the scores of a batch come back in one copy).  hyp_cap is set once all four hold that many
  Buf<char> hyp_dev; PinnedBuf<char> hyp_host; Buf<double> J_dev; PinnedBuf<double> J_host; int hyp_cap = 0;
  int *counts_dev() const { return (int *)(J_dev + hyp_cap); }
  int *counts_host() const { return (int *)(J_host + hyp_cap); }
  Buf<double> d_dev, gain_dev;                          // [len_cap][hyp_cap], reserved together
  bool counts_dirty = false;                            // a scoring round did not complete: counts_dev is cleared before the next one
  PinnedBuf<double> row_host;
  Buf<double> aux_dev;                                  // second point set (off-plane correspondences of rFtH)
  // two-point candidates of rFtH as index pairs and their counts: two slots of cand_cap candidates each (a block is counted while
  // the next one is drawn), an event per slot behind its count's copy back.  The host writes and reads them in place (mapped
  // memory); *_dev is the device address of *_host and null whenever that is empty
  MappedBuf<unsigned int> cand_host; MappedBuf<int> candc_host; int cand_cap = 0;
  unsigned int *cand_dev = nullptr; int *candc_dev = nullptr;
  hipEvent_t cand_ev[2] = {nullptr, nullptr};
  // models counted over all correspondences in one launch (innerFH's samples): k x 9 doubles in, k x COUNT_PARTS partial counts out,
  // both in mapped host memory
  MappedBuf<double> cntf_host; MappedBuf<int> cntc_host; int cntf_cap = 0;
  double *cntf_dev = nullptr; int *cntc_dev = nullptr;
  double score_ms = 0; long launches = 0;
  ~RansacGpu();                                         // events and the stream; the buffers free themselves
};

// A workspace of the calling thread, made at its first use.  A worker thread returns its HBM when it ends; the main thread's copy
// would be destroyed during process exit, when the HIP runtime (or a profiler layered on it) may already be shutting down and a
// hipFree can block forever - the process is going away, so the main thread's workspace is leaked on purpose.
template <class W> struct ThreadWorkspace {
  W *ws = nullptr;
  W &get() { if (!ws) ws = new W(); return *ws; }
  ~ThreadWorkspace() { if ((long)getpid() != (long)syscall(SYS_gettid)) delete ws; }
};
enum { HYP_SLOT_BYTES = 27 * 8 };   // largest hypothesis record (homography + its two symmetric operands)

RansacGpu *ransac_gpu();                                  // nullptr + mods_last_error when no device
bool ransac_ws_reserve(RansacGpu *ws, int len, int n_hyp);
bool ransac_fetch_row(RansacGpu *ws, int len, int k, double *dst);
bool ransac_counts_begin(RansacGpu *ws);                 // start of a scoring round (clears counters a failed round left behind)
long ransac_pinned_seed();                                // >= 0: pinned (mods_ransac_pin_seed / MODS_RANSAC_SEED)

// lane k adds gain[i][k], i = 0..len-1, in correspondence order (the MSAC score is a sequential sum)
__global__ void ransac_gain_kernel(const double *__restrict__ gain, int len, int n_hyp, int kstride, int *__restrict__ counts,
                                   double *__restrict__ J_out, int *__restrict__ counts_out);

// A device failure inside the control loops unwinds to the extern "C" entry point (the reference's signatures have no
// error channel): the entry point returns "no model" and raises the calling thread's failure flag, which
// mods_loransac_h / mods_loransac_f turn into MODS_E_HIP; the message is in mods_last_error().
struct RansacDeviceError {};
[[noreturn]] inline void ransac_fail() { throw RansacDeviceError(); }
void ransac_set_failed(int failed);       // calling thread's flag
int ransac_failed();

#define RS_CHECK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { set_error("%s failed: %s", #expr, hipGetErrorString(_e)); return false; } } while (0)

}  // namespace mods
