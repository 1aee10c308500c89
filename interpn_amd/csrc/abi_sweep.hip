// Sweep evaluation of large device-resident batches (linear_sweep.h, sweep_rounds.h): which of the four kernel families,
// the scratch block with the launch's work words, per stream, the device-side sample in front of automatic launches, and the
// decision to take the path.  (C ABI internals, see abi_internal.h.)
#include "abi_internal.h"

using namespace interpn;
using namespace interpn_abi;

namespace interpn {

int sweep_applies(const GridDesc& g, size_t npts) {
  if (g.method == kNearest) return nearest_sweep_applies(g, npts);  // 2-D / 3-D nearest neighbour: k_nearest.hip
  if (g.method == kCubic) return cubic_sweep_applies(g, npts);      // 2-D / 3-D multicubic: k_cubic_sweep.hip
  if (g.ndims == 2) return linear2_sweep_applies(g, npts);          // 2-D multilinear: k_linear2_brick.hip
  return linear3_sweep_applies(g, npts);                            // 3-D multilinear: k_linear_sweep.hip
}

hipError_t launch_sweep(const GridDesc& g, const void* const* obs, void* out, size_t npts, unsigned long long* first_bad,
                        void* work, hipStream_t stream) {
  if (!work || npts == 0) return hipErrorInvalidValue;
  if (g.method == kNearest) return launch_nearest_sweep(g, obs, out, npts, first_bad, work, stream);
  if (g.method == kCubic) return launch_cubic_sweep(g, obs, out, npts, first_bad, work, stream);
  if (g.ndims == 2) return launch_linear2_sweep(g, obs, out, npts, first_bad, work, stream);
  return launch_linear3_sweep(g, obs, out, npts, first_bad, work, stream);
}

}  // namespace interpn

namespace interpn_abi {

namespace {

// What an automatic launch through a scratch block runs.
struct SampleChoice {
  bool sample = false;            // the sampling kernel, then the sweep and the one-pass kernel, both gated by its verdict
  bool one_pass_only = false;     // no sample: the one-pass kernel alone
  unsigned* host_word = nullptr;  // where the sample also leaves its verdict for the host (null: nowhere)
  unsigned seq = 0;               // ... numbered so
};

// Decides the sample of this launch (handle's sampling state, under bin_mu); where a sample's verdict will be is noted once the
// launch has its scratch block.
// Thinned-out sampling (option sweep_probe = 2): a handle whose last three samples all said "unordered" is sampled on every
// 16th automatic launch only (the sample and the gated launch behind the sweep kernel cost ~1.5 % of a 1e8-point launch),
// and one whose last three said "coherent" runs the one-pass kernel alone in between; one verdict the other way brings every
// launch's sample back.  Whichever kernel runs, the results are the same bits.
SampleChoice choose_sample(interpn_hip_interp* h, size_t npoints) {
  const GridDesc& g = h->desc;
  SampleChoice c;
  c.sample = sweep_probe_applies(g) && npoints >= 256u * 64u;
  std::lock_guard<std::mutex> lk(h->bin_mu);
  interpn_hip_interp::SweepSampling& s = h->sampling;
  if (c.sample && g.cfg.sweep_probe == 2) {
    if (!s.host) {
      void* dp = nullptr;
      if (pool_take_pinned_word(h->device, &s.host) == hipSuccess && s.host &&
          hipHostGetDevicePointer(&dp, s.host, 0) == hipSuccess && dp) {
        *(volatile unsigned long long*)s.host = 0;
        s.host_dev = static_cast<unsigned*>(dp);
      } else {
        (void)hipGetLastError();
        s.host_dev = nullptr;
      }
    }
    if (s.host_dev) {
      const unsigned w = (unsigned)*(volatile unsigned long long*)s.host;
      if ((w >> 1) != s.seen && (w >> 1) != 0) {
        s.seen = w >> 1;
        s.streak = (w & 1u) ? 0 : s.streak + 1;
        s.streak_coherent = (w & 1u) ? s.streak_coherent + 1 : 0;
      }
      if ((s.streak >= 3 || s.streak_coherent >= 3) && s.skipped < 15) {
        ++s.skipped;
        c.sample = false;
        c.one_pass_only = s.streak < 3;  // (the last three said "coherent")
      } else {
        s.skipped = 0;
        s.seq = s.seq >= 0x7FFFFFFEu ? 1u : s.seq + 1u;
        c.host_word = s.host_dev;
        c.seq = s.seq;
      }
    }
  }
  s.last_word = nullptr;
  return c;
}

}  // namespace

// Returns -1 when the path does not apply or cannot be taken right now (`*why` says which; the
// caller then launches the one-pass kernel on the points as they are), otherwise a status.  The work
// words (1.25 KiB: round counters, the period measurement) live in a scratch block of the handle,
// taken per stream exactly like the sorted path's blocks (take_bin_slot): two streams never share
// one in flight.  Not taken while the stream is being captured into a graph (the block's event
// cannot be recorded there), for batches that give a wave fewer than four rounds, or for streams
// that are not 16-byte aligned.  A launch that runs the one-pass kernel alone (a handle in a streak of coherent batches)
// needs no work words: it takes no block and puts nothing but its kernel on the stream.
int eval_device_sweep(interpn_hip_interp* h, const void* const* obs, void* out, size_t npoints, hipStream_t stream,
                      unsigned flags, int* why) {
  const GridDesc& g = h->desc;
  *why = INTERPN_HIP_WHY_NONE;
  const int applies = sweep_applies(g, npoints);
  if (applies < 2) { *why = applies ? INTERPN_HIP_WHY_SMALL_OR_OFF : INTERPN_HIP_WHY_NONE; return -1; }
  if (reinterpret_cast<uintptr_t>(out) % 16) { *why = INTERPN_HIP_WHY_MISALIGNED; return -1; }
  for (int d = 0; d < g.ndims; ++d)
    if (reinterpret_cast<uintptr_t>(obs[d]) % 16) { *why = INTERPN_HIP_WHY_MISALIGNED; return -1; }
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); *why = INTERPN_HIP_WHY_CAPTURE; return -1; }
  if (cs != hipStreamCaptureStatusNone) { *why = INTERPN_HIP_WHY_CAPTURE; return -1; }
  // automatic mode: the device decides between the sweep kernel and the one-pass kernel (k_linear_sweep.hip::k_sweep_probe:
  // a sampling kernel in front, verdict 1 / 0 in the scratch block); both launches work from private copies of the
  // description that carry the gate (the handle's own is shared by threads)
  const SampleChoice c = choose_sample(h, npoints);
  if (c.one_pass_only) {
    GridDesc gb = g;
    gb.launch_fat = true;  // (the workgroup shape of the gated launch: what coherent batches run best in)
    const hipError_t e1 = launch_any(gb, obs, out, npoints, h->first_bad, stream);
    g.tag = gb.tag;
    if (e1 != hipSuccess) {
      (void)hipGetLastError();
      return hip_fail(e1);
    }
    return INTERPN_HIP_OK;
  }
  interpn_hip_interp::BinSlot* slot = take_bin_slot(h, sweep_work_bytes(), stream, !(flags & INTERPN_HIP_EVAL_NO_ALLOC), why);
  if (!slot) return -1;
  if (c.sample) {
    std::lock_guard<std::mutex> lk(h->bin_mu);
    h->sampling.last_word = static_cast<const unsigned char*>(slot->scratch) + sweep_probe_word_offset();
  }
  hipError_t err = hipSuccess;
  // first use of the block by this path, or the sorted path has used it since: reset the work words (a complete launch leaves
  // its counters zero and its measured period in place; that period word is one of the sort's bin counters)
  if (!slot->sweep_clean) err = hipMemsetAsync(slot->scratch, 0, sweep_work_bytes(), stream);
  if (c.sample && err == hipSuccess) err = launch_sweep_probe(g, obs, npoints, slot->scratch, stream, c.host_word, c.seq);
  if (err == hipSuccess) {
    if (c.sample) {
      GridDesc gs = g;
      gs.sweep_gated = true;
      err = launch_sweep(gs, obs, out, npoints, h->first_bad, slot->scratch, stream);
      g.tag = gs.tag;  // the handle reports the sweep kernel (which of the pair ran is known on the device only: option sweep_probe_took_brick)
    } else {
      err = launch_sweep(g, obs, out, npoints, h->first_bad, slot->scratch, stream);
    }
  }
  if (c.sample && err == hipSuccess) {
    GridDesc gb = g;
    gb.launch_gate = reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(slot->scratch) + sweep_probe_word_offset());
    err = launch_any(gb, obs, out, npoints, h->first_bad, stream);
  }
  slot->sweep_clean = err == hipSuccess;
  slot->totals_clean = false;
  release_bin_slot(h, slot, stream, /*staged=*/false);
  if (err != hipSuccess) {
    (void)hipGetLastError();
    return hip_fail(err);
  }
  return INTERPN_HIP_OK;
}

}  // namespace interpn_abi
