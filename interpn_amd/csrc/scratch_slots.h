// Scratch blocks between streams, and the streams a handle must wait for: the decisions, with no HIP in them.
//
// A handle owns up to kMaxBinSlots scratch blocks that every evaluation through it shares.  Two streams never work in
// a block at the same time, and a block is freed only once its last use is complete — without a command on any
// stream behind a launch: a block remembers the stream that used it last, and its event is recorded behind that use
// only when somebody needs it (settle_slot): another stream that takes the block, or a block about to be freed.
// Likewise a launch only notes its stream (mark_stream), and destroying the handle waits for the noted streams.
//
// Everything here is written against a runtime type RT, so that the same text runs on HIP (abi_internal.h:
// HipRuntime, whose members forward one to one to hip* and the per-device pool) and on a model of streams that can
// tell which use happens before which (tests/test_scratch_slots_cpu.py).  RT supplies
//   types   Stream, Event (copyable, comparable with ==)
//   const   kNotReady: what event_query returns while the event is pending
//   calls   returning 0 on success:
//           is_capturing(Stream, bool*)    event_create(Event*)       event_destroy(Event)
//           event_record(Event, Stream)    event_query(Event)         event_synchronize(Event)
//           stream_wait_event(Stream, Event)   stream_synchronize(Stream)   device_synchronize()
//           alloc_block(void**, size_t)
//   and     clear_last_error(), free_block(void*) (null: nothing).
//
// What the model checks, after every operation (I1–I7):
//   I1  a use of a block is enqueued only if every earlier use of the same allocation happens-before it
//   I2  an allocation is freed or regrown only after the host knows every use of it complete
//   I3  a stream under capture is only ever asked whether it is; a block whose last stream is capturing goes to nobody else
//   I4  reuse of a block by the stream that used it last: no command on any stream, no event call
//   I5  after destroy_wait every use enqueued through the table is complete; the device is synchronised only for
//       more than kMaxMarks streams, a captured or a destroyed one, or a launch that could not be marked
//   I6  at most kMaxBinSlots blocks; no allocation where it is forbidden; a failed allocation or event creation says
//       so and leaves the table usable; everything allocated or created is given back (free_blocks)
//   I7  a block whose last stream has been destroyed: no event can be recorded, so the device is synchronised before
//       the block is reused, and again at destroy
// Not covered, the caller's to keep: a stream destroyed with work of this handle in flight on it, whose handle VALUE
// the runtime then gives to a new stream, looks like the same stream to step 1 of take_bin_slot and to mark_stream.
// Synchronise a stream (or finish on it) before destroying it.  (HIP on ROCm drains a stream in hipStreamDestroy.)
#pragma once
#include <atomic>
#include <cstddef>
#include <mutex>
#include <vector>

#include "../../include/interpn_hip.h"

namespace scratch_slots {

template <class RT>
struct Slot {
  void* scratch = nullptr;
  size_t bytes = 0;
  typename RT::Event event{};
  bool recorded = false;       // `event` has been recorded behind the block's last use
  bool unmarked = false;       // the last use may be in flight on `last_stream` with no event behind it yet (settle_slot)
  bool busy = false;           // a host thread is enqueueing into this block right now
  typename RT::Stream last_stream{};
  unsigned long long stamp = 0;  // use counter value of the last use (LRU)
  bool totals_clean = false;     // the block's bin counters are zero (left so by the last complete sort's scan)
  // the block's first sweep_work_bytes() are a SweepWork a complete sweep launch left behind (round counters zero, the
  // measured period kept for the next launch).  The two invariants exclude each other: the period word lies inside the
  // sort's histogram (totals[291]), so whichever path uses a block clears the other path's flag.
  bool sweep_clean = false;
  typename RT::Event stage[5] = {};  // option stage_timing: start | hist | scan | scatter | kernel
  bool staged = false;               // the last use recorded them (single slice)
};

// The part of a handle this header works on (interpn_hip_interp derives from it).
template <class RT>
struct Table {
  using Runtime = RT;
  using BinSlot = Slot<RT>;
  static constexpr size_t kMaxBinSlots = 4;
  static constexpr size_t kMaxMarks = 16;
  RT rt;
  // `bin_mu` guards the slot list (and, in the handle, the per-handle report fields); launches are enqueued outside it.
  std::mutex bin_mu;
  std::vector<BinSlot> bin_slots;  // capacity kMaxBinSlots from the start: evaluations hold pointers to elements outside the lock
  unsigned long long bin_uses = 0;
  std::atomic<long long> scratch_allocs{0};
  const void** word_in_block = nullptr;  // (guarded by bin_mu) a pointer into some block that the owner keeps: cleared when a block is freed
  // Caller streams that device-pointer work was enqueued on: destroy_wait waits for exactly these instead of stalling
  // the whole device.  `sync_device_at_destroy` is set for launches that could not be marked (a stream under capture,
  // more than kMaxMarks streams) and for streams that cannot be waited for any more (destroyed by the caller).
  std::mutex marks_mu;
  std::vector<typename RT::Stream> marks;
  bool sync_device_at_destroy = false;
  Table() { bin_slots.reserve(kMaxBinSlots); }
};

// (bin_mu held) Makes the block's last use known to the runtime: records the block's event on the stream of that use,
// which covers everything that stream holds by now.  Afterwards `recorded` says whether there is an event to wait for
// (none: the block was never used, or its stream is gone and the device has been waited for instead).  False: that
// stream is being captured and must not be touched — the block cannot be handed to anybody else right now.
template <class T>
bool settle_slot(T& t, typename T::BinSlot& sl) {
  if (!sl.unmarked) return true;
  bool capturing = false;
  int e = t.rt.is_capturing(sl.last_stream, &capturing);
  if (e == 0 && capturing) return false;
  if (e == 0) e = t.rt.event_record(sl.event, sl.last_stream);
  sl.unmarked = false;
  sl.recorded = e == 0;
  if (e != 0) {
    // no event behind the work (the caller has destroyed that stream, say): make it complete before anyone reuses the block
    t.rt.clear_last_error();
    if (t.rt.device_synchronize() != 0) t.rt.clear_last_error();
    std::lock_guard<std::mutex> lk(t.marks_mu);
    t.sync_device_at_destroy = true;
  }
  return true;
}

// Take a scratch block of at least `need` bytes for an evaluation on `stream`.  On success the block is marked busy
// and, where another stream used it last, `stream` has been made to wait for that use (whose event is recorded at
// this moment, not when the use ended).  `*why` (INTERPN_HIP_WHY_*) says why not otherwise.
template <class T>
typename T::BinSlot* take_bin_slot(T& t, size_t need, typename T::Runtime::Stream stream, bool may_alloc, int* why) {
  using BinSlot = typename T::BinSlot;
  std::unique_lock<std::mutex> lk(t.bin_mu);  // (step 5 drops it around a wait)
  BinSlot* pick = nullptr;
  bool wait = false;
  for (auto& sl : t.bin_slots) {  // 1. the block this stream used last: stream order is enough
    if (sl.busy || sl.bytes < need || !(sl.recorded || sl.unmarked)) continue;
    if (sl.last_stream == stream) { pick = &sl; break; }
  }
  if (!pick)
    for (auto& sl : t.bin_slots) {  // 2. an idle block
      if (sl.busy || sl.bytes < need || !settle_slot(t, sl)) continue;
      if (!sl.recorded) { pick = &sl; break; }
      const int q = t.rt.event_query(sl.event);
      if (q == 0) { pick = &sl; break; }
      if (q != T::Runtime::kNotReady) t.rt.clear_last_error();
    }
  if (!pick && may_alloc && t.bin_slots.size() < T::kMaxBinSlots) {  // 3. a new block
    BinSlot sl;
    if (t.rt.event_create(&sl.event) != 0) { t.rt.clear_last_error(); *why = INTERPN_HIP_WHY_ALLOC_FAILED; return nullptr; }
    if (t.rt.alloc_block(&sl.scratch, need) != 0) {
      t.rt.clear_last_error();
      (void)t.rt.event_destroy(sl.event);
      *why = INTERPN_HIP_WHY_ALLOC_FAILED;
      return nullptr;
    }
    sl.bytes = need;
    t.scratch_allocs.fetch_add(1);
    t.bin_slots.push_back(sl);
    pick = &t.bin_slots.back();
  }
  // (from here on every candidate has been through settle_slot in step 2: `unmarked` means its stream is being captured)
  if (!pick) {  // 4. the least recently used block that is large enough: wait for it on the device
    for (auto& sl : t.bin_slots)
      if (!sl.busy && !sl.unmarked && sl.bytes >= need && (!pick || sl.stamp < pick->stamp)) pick = &sl;
    wait = pick != nullptr;
  }
  if (!pick && may_alloc) {  // 5. grow the least recently used block that nobody is enqueueing into
    for (auto& sl : t.bin_slots)
      if (!sl.busy && settle_slot(t, sl) && (!pick || sl.stamp < pick->stamp)) pick = &sl;
    if (pick) {
      // The block's last use must complete before it is freed.  That wait and the reallocation run WITHOUT the lock
      // (the slot is marked busy, so nobody else takes it): other threads keep enqueueing through this table
      // meanwhile.  Growth is synchronous for the caller — reserve_blocks avoids it.
      pick->busy = true;
      const bool recorded = pick->recorded;
      const typename T::Runtime::Event ev = pick->event;
      void* const old = pick->scratch;
      lk.unlock();
      bool freed = false;
      void* fresh = nullptr;
      bool ok = !recorded || t.rt.event_synchronize(ev) == 0;
      if (ok) {
        t.rt.free_block(old);
        freed = true;
        ok = t.rt.alloc_block(&fresh, need) == 0;
      }
      if (!ok) t.rt.clear_last_error();
      lk.lock();
      if (freed && t.word_in_block) *t.word_in_block = nullptr;
      pick->busy = false;
      if (!ok) {
        if (freed) { pick->scratch = nullptr; pick->bytes = 0; pick->recorded = false; }  // else the old block stays as it was
        pick->totals_clean = false;
        pick->sweep_clean = false;
        *why = INTERPN_HIP_WHY_ALLOC_FAILED;
        return nullptr;
      }
      pick->scratch = fresh;
      pick->bytes = need;
      pick->totals_clean = false;
      pick->sweep_clean = false;
      pick->recorded = false;
      t.scratch_allocs.fetch_add(1);
    }
  }
  if (!pick) { *why = INTERPN_HIP_WHY_NO_SCRATCH; return nullptr; }
  if (pick->recorded && !(pick->last_stream == stream)) {  // (after step 2 or 5 the event is complete already: the wait is free)
    const int e = t.rt.stream_wait_event(stream, pick->event);
    if (wait && e != 0) { t.rt.clear_last_error(); *why = INTERPN_HIP_WHY_NO_SCRATCH; return nullptr; }
  }
  pick->busy = true;
  pick->stamp = ++t.bin_uses;
  return pick;
}

// Ends an evaluation's use of a block from take_bin_slot.  Nothing goes onto the stream: the block remembers the
// stream, and whoever needs an event behind this use — also behind a sequence cut short by a failure — records it then
// (settle_slot).  `staged`: the block's stage events were recorded by this use (option stage_timing).
template <class T>
void release_bin_slot(T& t, typename T::BinSlot* slot, typename T::Runtime::Stream stream, bool staged) {
  std::lock_guard<std::mutex> lk(t.bin_mu);
  slot->unmarked = true;
  slot->recorded = false;
  slot->last_stream = stream;
  slot->busy = false;
  slot->staged = staged;
}

// Under graph capture no event of a block may be queried, waited for or recorded (the captured launch may replay at
// any later time): take a block that is large enough without any of that — no runtime call at all.  The caller keeps
// other streams away from the handle while such a graph replays (include/interpn_hip.h).
template <class T>
typename T::BinSlot* take_slot_captured(T& t, size_t need, typename T::Runtime::Stream stream) {
  std::lock_guard<std::mutex> lk(t.bin_mu);
  typename T::BinSlot* pick = nullptr;
  for (auto& sl : t.bin_slots) {
    if (sl.busy || sl.bytes < need) continue;
    if (!pick || sl.last_stream == stream) pick = &sl;
  }
  if (pick) {
    pick->busy = true;
    pick->stamp = ++t.bin_uses;
  }
  return pick;
}

template <class T>
void release_slot_captured(T& t, typename T::BinSlot* slot) {
  std::lock_guard<std::mutex> lk(t.bin_mu);
  slot->busy = false;
}

// Makes sure `nstreams` blocks of at least `need` bytes exist: grows idle blocks that are too small first, then adds
// new ones.  Synchronous (a block in flight is waited for before it is freed).  Returns INTERPN_HIP_OK,
// INTERPN_HIP_ERR_OUT_OF_MEMORY, or -1 with the runtime's error in *rt_error.
template <class T>
int reserve_blocks(T& t, size_t need, int nstreams, int* rt_error) {
  std::lock_guard<std::mutex> lk(t.bin_mu);
  int have = 0;
  for (auto& sl : t.bin_slots)
    if (sl.bytes >= need) ++have;
  for (auto& sl : t.bin_slots) {
    if (have >= nstreams) break;
    if (sl.bytes >= need || sl.busy || !settle_slot(t, sl)) continue;
    if (sl.recorded) {
      const int e = t.rt.event_synchronize(sl.event);
      if (e != 0) { *rt_error = e; return -1; }
    }
    t.rt.free_block(sl.scratch);
    if (t.word_in_block) *t.word_in_block = nullptr;
    sl.scratch = nullptr;
    sl.bytes = 0;
    sl.totals_clean = false;
    sl.sweep_clean = false;
    sl.recorded = false;
    if (t.rt.alloc_block(&sl.scratch, need) != 0) { t.rt.clear_last_error(); sl.scratch = nullptr; return INTERPN_HIP_ERR_OUT_OF_MEMORY; }
    sl.bytes = need;
    t.scratch_allocs.fetch_add(1);
    ++have;
  }
  while (have < nstreams && t.bin_slots.size() < T::kMaxBinSlots) {
    typename T::BinSlot sl;
    const int e = t.rt.event_create(&sl.event);
    if (e != 0) { *rt_error = e; return -1; }
    if (t.rt.alloc_block(&sl.scratch, need) != 0) { t.rt.clear_last_error(); (void)t.rt.event_destroy(sl.event); return INTERPN_HIP_ERR_OUT_OF_MEMORY; }
    sl.bytes = need;
    t.scratch_allocs.fetch_add(1);
    t.bin_slots.push_back(sl);
    ++have;
  }
  return have >= nstreams ? INTERPN_HIP_OK : INTERPN_HIP_ERR_OUT_OF_MEMORY;
}

// Remember that device-pointer work was enqueued on `stream`.  No allocation, copy, synchronisation or stream
// command: the stream is noted, and destroy_wait waits for it.  A stream under capture is never touched.
template <class T>
void mark_stream(T& t, typename T::Runtime::Stream stream) {
  bool capturing = false;
  if (t.rt.is_capturing(stream, &capturing) != 0) {
    t.rt.clear_last_error();
    std::lock_guard<std::mutex> lk(t.marks_mu);
    t.sync_device_at_destroy = true;
    return;
  }
  std::lock_guard<std::mutex> lk(t.marks_mu);
  if (capturing) {
    t.sync_device_at_destroy = true;  // the graph may replay this launch at any later time
    return;
  }
  for (const auto& m : t.marks)
    if (m == stream) return;
  if (t.marks.size() >= T::kMaxMarks) {
    t.sync_device_at_destroy = true;
    return;
  }
  t.marks.push_back(stream);
}

// What destroying a handle waits for before its blocks go back: the caller streams it enqueued on, then the owner's
// own streams (`own_streams()`: false if one of them could not be waited for) — not the whole device: unrelated
// streams keep running.  Launches put no marker on their stream, so the wait covers what a stream holds now.
// Launches that could not be marked, a stream the caller has destroyed since and one that is being captured (never
// touched) fall back to synchronising the device.
template <class T, class Own>
void destroy_wait(T& t, Own&& own_streams) {
  {
    std::lock_guard<std::mutex> lk(t.marks_mu);
    for (const auto& m : t.marks) {
      bool capturing = false;
      int e = t.rt.is_capturing(m, &capturing);
      if (e == 0 && !capturing) e = t.rt.stream_synchronize(m);
      if (e != 0 || capturing) {
        t.rt.clear_last_error();
        t.sync_device_at_destroy = true;
      }
    }
    t.marks.clear();
  }
  if (!own_streams()) t.sync_device_at_destroy = true;
  if (t.sync_device_at_destroy) (void)t.rt.device_synchronize();
}

// (after destroy_wait) Gives every block and event back; `per_slot(slot)` runs between a slot's event and its block.
template <class T, class PerSlot>
void free_blocks(T& t, PerSlot&& per_slot) {
  for (auto& sl : t.bin_slots) {
    if (!(sl.event == typename T::Runtime::Event{})) (void)t.rt.event_destroy(sl.event);
    per_slot(sl);
    t.rt.free_block(sl.scratch);
  }
  t.bin_slots.clear();
}

}  // namespace scratch_slots
