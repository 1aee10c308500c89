"""The rules that keep a handle's scratch blocks apart between streams (interpn_amd/csrc/scratch_slots.h: settle, the
five steps of take, release, the captured take, reserve, stream marks and the wait at destroy), run against a MODEL
of streams instead of HIP.  No GPU.

The model's streams are FIFO queues of commands (use of a block, event record, wait for an event) with a cursor
"the device has completed up to here" that the test moves, a capture state and a destroyed state.  It keeps the
happens-before relation over the commands as vector clocks: stream order, record -> wait edges, and everything a
host-side synchronise or a successful event query has shown complete happens-before whatever is enqueued afterwards.
The invariants I1-I7 (listed in the header) are checked on that RELATION, after every operation, so they hold for
every schedule of the device and not for one interleaving.

Inputs: named scenarios, one per step of take_bin_slot and per special case; a seeded random walk of 20 000
operations over six streams, three seeds; four host threads through one table, built with -fsanitize=thread and with
-fsanitize=address,undefined as a stand-alone program.  And the test's own teeth: seven one-line mutants of the
header, each of which the scenarios must reject, naming the invariant.

A decision pinned here (scenario `stream_value_reused`): step 1 of take and the stream marks know a stream by its
handle's value.  A caller that destroys a stream with work of the handle in flight and is handed the same value for a
new stream gets "same stream" reuse with nothing in between, and nothing in settle or the marks sees it (neither is
asked on that path — that is the point of step 1).  The library does not cover this; the caller synchronises a
stream before destroying it (HIP on ROCm drains the stream in hipStreamDestroy anyway).  The scenario shows both
halves: reuse after a synchronise is clean, reuse without one is an I1 violation that the model reports."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interpn_amd", "csrc")
HEADER = os.path.join(CSRC, "scratch_slots.h")
CXX = os.environ.get("CXX", "g++")

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "scratch_slots.h"

// ---------------------------------------------------------------------------------------------------------------
// The model runtime.
struct MStream { int value = -1; bool operator==(const MStream& o) const { return value == o.value; } };
struct MEvent { int id = -1; bool operator==(const MEvent& o) const { return id == o.id; } };

static const char* g_scenario = "";
static unsigned g_seed = 0;
static long g_op = -1;
static std::string g_expect;      // an invariant whose violation the scenario expects (and then requires)
static bool g_expected_seen = false;

static void violation(const char* inv, const std::string& what) {
  if (!g_expect.empty() && g_expect == inv) { g_expected_seen = true; return; }
  std::printf("VIOLATION %s: %s (scenario %s, seed %u, operation %ld)\n", inv, what.c_str(), g_scenario, g_seed, g_op);
  std::fflush(stdout);
  std::_Exit(1);
}
#define REQUIRE(cond, inv, what) do { if (!(cond)) violation(inv, what); } while (0)

enum Kind { kUse, kRecord, kWait };
struct Cmd {
  int gen, pos, kind, alloc, record;  // record: the record command a wait waits for (-1: none)
  std::vector<int> vc;                // vc[g] = commands of stream g that happen-before this one (itself included)
};
struct Gen {  // one stream: a handle value the caller was given, until it is destroyed
  int value;
  bool destroyed = false, capturing = false;
  std::vector<int> cmds;
  size_t done = 0;
};

struct Model {
  std::mutex mu;
  std::vector<Gen> gens;
  std::map<int, int> by_value;        // handle value -> the stream that has it now
  std::vector<Cmd> cmds;
  std::vector<int> known;             // per stream: how many of its commands the HOST knows complete
  std::vector<int> event_record;      // per event: its latest record command (-1: never recorded)
  std::vector<std::vector<int>> use_clock;  // per allocation: per stream, commands up to its last use there
  std::vector<bool> live;
  long calls = 0, event_calls = 0, commands = 0, capture_queries = 0, device_syncs = 0, allocs = 0, frees = 0;
  long events_created = 0, events_destroyed = 0, live_blocks = 0, uses = 0;
  int fail_alloc_in = 0, fail_event_in = 0;  // k: the k-th call from now fails
  bool failure_fired = false;
  bool alloc_forbidden = false;
  bool dead_stream_answers_query = false;  // the capture query of a destroyed stream succeeds (every other call on it fails)

  // ---- streams (the test's side)
  MStream create(int value) {
    std::lock_guard<std::mutex> lk(mu);
    Gen g;
    g.value = value;
    gens.push_back(g);
    known.push_back(0);
    by_value[value] = (int)gens.size() - 1;
    return MStream{value};
  }
  int lookup(MStream s) {  // the live stream behind a handle value, or -1
    auto it = by_value.find(s.value);
    if (it == by_value.end() || gens[it->second].destroyed) return -1;
    return it->second;
  }
  void destroy_stream(MStream s) {  // (what it holds stays in flight)
    std::lock_guard<std::mutex> lk(mu);
    const int g = lookup(s);
    if (g >= 0) { gens[g].destroyed = true; gens[g].capturing = false; }
  }
  void set_capture(MStream s, bool on) {
    std::lock_guard<std::mutex> lk(mu);
    const int g = lookup(s);
    if (g >= 0) gens[g].capturing = on;
  }
  bool capturing(MStream s) {
    std::lock_guard<std::mutex> lk(mu);
    const int g = lookup(s);
    return g >= 0 && gens[g].capturing;
  }

  // ---- the device
  bool complete(int c) const { return (size_t)cmds[c].pos < gens[cmds[c].gen].done; }
  void advance(int g, int k) {  // the device completes up to k more commands of stream g, as far as their waits allow
    Gen& s = gens[g];
    while (k-- > 0 && s.done < s.cmds.size()) {
      const Cmd& c = cmds[s.cmds[s.done]];
      if (c.kind == kWait && c.record >= 0 && !complete(c.record)) break;
      ++s.done;
    }
  }
  void force(int c) {  // a host-side wait: the device runs until command c is complete
    const int g = cmds[c].gen;
    while (gens[g].done <= (size_t)cmds[c].pos) {
      const Cmd& next = cmds[gens[g].cmds[gens[g].done]];
      if (next.kind == kWait && next.record >= 0 && !complete(next.record)) force(next.record);
      ++gens[g].done;
    }
  }
  void learn(int c) {  // the host has seen command c complete: so is everything that happens-before it
    for (size_t j = 0; j < cmds[c].vc.size(); ++j) known[j] = std::max(known[j], cmds[c].vc[j]);
  }
  int enqueue(int g, int kind, int alloc, int record) {
    Cmd c{g, (int)gens[g].cmds.size(), kind, alloc, record, {}};
    c.vc = known;  // what the host knows complete happens-before everything enqueued afterwards
    c.vc.resize(gens.size(), 0);
    auto join = [&](const std::vector<int>& o) { for (size_t j = 0; j < o.size(); ++j) c.vc[j] = std::max(c.vc[j], o[j]); };
    if (!gens[g].cmds.empty()) join(cmds[gens[g].cmds.back()].vc);
    if (kind == kWait && record >= 0) join(cmds[record].vc);
    if (kind == kUse) {  // I1, before the command counts itself
      REQUIRE(live[alloc], "I2", "a use of an allocation that has been freed");
      for (size_t j = 0; j < use_clock[alloc].size(); ++j)
        REQUIRE(use_clock[alloc][j] <= c.vc[j], "I1",
                "a use on stream " + std::to_string(gens[g].value) + " with an earlier use of the same allocation on stream " +
                    std::to_string(gens[j].value) + " not ordered before it");
    }
    c.vc[g] = c.pos + 1;
    if (kind == kUse) {
      use_clock[alloc].resize(gens.size(), 0);
      use_clock[alloc][g] = c.pos + 1;
      ++uses;
    }
    cmds.push_back(c);
    gens[g].cmds.push_back((int)cmds.size() - 1);
    return (int)cmds.size() - 1;
  }
  // the launch's kernels: a use of `block` on `s` (the test's side: not a call of the code under test)
  void use(MStream s, void* block) {
    std::lock_guard<std::mutex> lk(mu);
    const int g = lookup(s);
    REQUIRE(g >= 0, "TEST", "launch on a dead stream");
    enqueue(g, kUse, (int)((size_t)block >> 12) - 1, -1);
  }
  void host_sync(MStream s) {  // the CALLER synchronises a stream
    std::lock_guard<std::mutex> lk(mu);
    const int g = lookup(s);
    if (g < 0 || gens[g].capturing || gens[g].cmds.empty()) return;
    force(gens[g].cmds.back());
    learn(gens[g].cmds.back());
  }
  bool all_uses_complete() const {
    for (size_t c = 0; c < cmds.size(); ++c)
      if (cmds[c].kind == kUse && !complete((int)c)) return false;
    return true;
  }

  // ---- the runtime calls of scratch_slots.h (each under the model's own mutex)
  int on_stream(MStream s, const char* what) {  // the stream a call other than the capture query works on, or -1 = the call fails
    const int g = lookup(s);
    if (g < 0) return -1;
    if (gens[g].capturing) { violation("I3", std::string(what) + " on a stream under capture"); return -1; }
    return g;
  }
  int is_capturing(MStream s, bool* cap) {
    std::lock_guard<std::mutex> lk(mu);
    ++calls; ++capture_queries;
    const int g = lookup(s);
    if (g < 0 && dead_stream_answers_query) { *cap = false; return 0; }
    if (g < 0) return 1;
    *cap = gens[g].capturing;
    return 0;
  }
  int event_create(MEvent* ev) {
    std::lock_guard<std::mutex> lk(mu);
    ++calls; ++event_calls;
    if (fail_event_in > 0 && --fail_event_in == 0) { failure_fired = true; return 2; }
    event_record.push_back(-1);
    ev->id = (int)event_record.size() - 1;
    ++events_created;
    return 0;
  }
  int event_destroy(MEvent) {
    std::lock_guard<std::mutex> lk(mu);
    ++calls; ++event_calls; ++events_destroyed;
    return 0;
  }
  int event_record_(MEvent ev, MStream s) {
    std::lock_guard<std::mutex> lk(mu);
    ++calls; ++event_calls;
    const int g = on_stream(s, "event record");
    if (g < 0) return 1;
    ++commands;
    event_record[ev.id] = enqueue(g, kRecord, -1, -1);
    return 0;
  }
  int event_query(MEvent ev) {
    std::lock_guard<std::mutex> lk(mu);
    ++calls; ++event_calls;
    const int r = event_record[ev.id];
    if (r >= 0 && !complete(r)) return 600;
    if (r >= 0) learn(r);
    return 0;
  }
  int event_synchronize(MEvent ev) {
    std::lock_guard<std::mutex> lk(mu);
    ++calls; ++event_calls;
    const int r = event_record[ev.id];
    if (r >= 0) { force(r); learn(r); }
    return 0;
  }
  int stream_wait_event(MStream s, MEvent ev) {
    std::lock_guard<std::mutex> lk(mu);
    ++calls; ++event_calls;
    const int g = on_stream(s, "wait for an event");
    if (g < 0) return 1;
    ++commands;
    enqueue(g, kWait, -1, event_record[ev.id]);
    return 0;
  }
  int stream_synchronize(MStream s) {
    std::lock_guard<std::mutex> lk(mu);
    ++calls;
    const int g = on_stream(s, "stream synchronise");
    if (g < 0) return 1;
    if (!gens[g].cmds.empty()) { force(gens[g].cmds.back()); learn(gens[g].cmds.back()); }
    return 0;
  }
  int device_synchronize() {
    std::lock_guard<std::mutex> lk(mu);
    ++calls; ++device_syncs;
    for (auto& g : gens)
      if (!g.cmds.empty()) { force(g.cmds.back()); learn(g.cmds.back()); }
    return 0;
  }
  void clear_last_error() {
    std::lock_guard<std::mutex> lk(mu);
    ++calls;
  }
  int alloc_block(void** out, size_t) {
    std::lock_guard<std::mutex> lk(mu);
    ++calls;
    REQUIRE(!alloc_forbidden, "I6", "an allocation where the caller forbade one");
    if (fail_alloc_in > 0 && --fail_alloc_in == 0) { failure_fired = true; return 3; }
    live.push_back(true);
    use_clock.emplace_back();
    ++allocs; ++live_blocks;
    REQUIRE(live_blocks <= 4, "I6", "more blocks than kMaxBinSlots");
    *out = (void*)(live.size() << 12);  // never reused: a use of a freed allocation shows
    return 0;
  }
  void free_block(void* p) {
    std::lock_guard<std::mutex> lk(mu);
    ++calls;
    if (!p) return;
    const int a = (int)((size_t)p >> 12) - 1;
    REQUIRE(live[a], "I2", "an allocation freed twice");
    for (size_t j = 0; j < use_clock[a].size(); ++j)
      REQUIRE(use_clock[a][j] <= known[j], "I2",
              "an allocation freed while the host does not know its use on stream " + std::to_string(gens[j].value) + " complete");
    live[a] = false;
    ++frees; --live_blocks;
  }
};

struct ModelRuntime {
  using Stream = MStream;
  using Event = MEvent;
  static constexpr int kNotReady = 600;
  Model* m = nullptr;
  int is_capturing(Stream s, bool* c) { return m->is_capturing(s, c); }
  int event_create(Event* e) { return m->event_create(e); }
  int event_destroy(Event e) { return m->event_destroy(e); }
  int event_record(Event e, Stream s) { return m->event_record_(e, s); }
  int event_query(Event e) { return m->event_query(e); }
  int event_synchronize(Event e) { return m->event_synchronize(e); }
  int stream_wait_event(Stream s, Event e) { return m->stream_wait_event(s, e); }
  int stream_synchronize(Stream s) { return m->stream_synchronize(s); }
  int device_synchronize() { return m->device_synchronize(); }
  void clear_last_error() { m->clear_last_error(); }
  int alloc_block(void** out, size_t bytes) { return m->alloc_block(out, bytes); }
  void free_block(void* p) { m->free_block(p); }
};
using Tab = scratch_slots::Table<ModelRuntime>;
using Slot = Tab::BinSlot;

// ---------------------------------------------------------------------------------------------------------------
// The driver: what a launch through the handle does around its kernels.
struct World {
  Model m;
  Tab t;
  bool threaded = false;
  World() { t.rt.m = &m; }

  struct Result { int slot = -1; int why = 0; long calls = 0, commands = 0, event_calls = 0; };

  Result launch(MStream s, size_t need, bool may_alloc) {
    Result r;
    const bool cap = m.capturing(s);
    if (threaded) return launch_threaded(s, need, may_alloc, cap);
    bool same_stream = false;
    bool held[8] = {false};
    if (!threaded) {
      for (size_t i = 0; i < t.bin_slots.size(); ++i) {
        const Slot& sl = t.bin_slots[i];
        held[i] = sl.unmarked && m.capturing(sl.last_stream);
        same_stream = same_stream || (!sl.busy && sl.bytes >= need && (sl.recorded || sl.unmarked) && sl.last_stream == s);
      }
    }
    const long calls0 = m.calls, commands0 = m.commands, events0 = m.event_calls, allocs0 = m.allocs;
    m.failure_fired = false;
    Slot* slot = nullptr;
    if (cap) {
      slot = scratch_slots::take_slot_captured(t, need, s);
      REQUIRE(threaded || m.calls == calls0, "I3", "the captured take made a runtime call");
    } else {
      m.alloc_forbidden = !may_alloc && !threaded;
      slot = scratch_slots::take_bin_slot(t, need, s, may_alloc, &r.why);
      m.alloc_forbidden = false;
      if (!threaded) {
        REQUIRE(may_alloc || m.allocs == allocs0, "I6", "an allocation where the caller forbade one");
        if (!slot)
          REQUIRE(r.why == (m.failure_fired ? INTERPN_HIP_WHY_ALLOC_FAILED : INTERPN_HIP_WHY_NO_SCRATCH), "I6",
                  "no block, and `why` = " + std::to_string(r.why) + " does not say what happened");
      }
    }
    if (slot) {
      r.slot = (int)(slot - t.bin_slots.data());
      if (!threaded && !cap)
        REQUIRE(!held[r.slot] || slot->last_stream == s, "I3", "a block whose last stream is under capture was handed to another stream");
      REQUIRE(slot->bytes >= need && slot->scratch, "I6", "a block smaller than asked for");
      if (!cap) m.use(s, slot->scratch);  // (a captured launch runs when its graph replays: the caller keeps others away then)
      if (cap) scratch_slots::release_slot_captured(t, slot);
      else scratch_slots::release_bin_slot(t, slot, s, false);
      scratch_slots::mark_stream(t, s);
    }
    r.calls = m.calls - calls0;
    r.commands = m.commands - commands0;
    r.event_calls = m.event_calls - events0;
    if (!threaded && same_stream && slot && !cap)  // (mark_stream asks whether the stream is capturing: that one call is the launch's, not the block's)
      REQUIRE(r.commands == 0 && r.event_calls == 0 && r.calls == 1, "I4", "reuse by the stream that used the block last touched the runtime");
    check();
    return r;
  }
  // (several host threads: the counters and the slots' fields are other threads' too, so only what the model itself checks
  // under its mutex — I1, I2, the block count of I6 — is checked)
  Result launch_threaded(MStream s, size_t need, bool may_alloc, bool cap) {
    Result r;
    Slot* slot = cap ? scratch_slots::take_slot_captured(t, need, s) : scratch_slots::take_bin_slot(t, need, s, may_alloc, &r.why);
    if (!slot) return r;
    r.slot = (int)(slot - t.bin_slots.data());
    REQUIRE(slot->bytes >= need && slot->scratch, "I6", "a block smaller than asked for");
    if (!cap) m.use(s, slot->scratch);
    if (cap) scratch_slots::release_slot_captured(t, slot);
    else scratch_slots::release_bin_slot(t, slot, s, false);
    scratch_slots::mark_stream(t, s);
    return r;
  }
  int reserve(size_t need, int nstreams) {
    int rt_error = 0;
    const int st = scratch_slots::reserve_blocks(t, need, nstreams, &rt_error);
    check();
    return st;
  }
  void check() {
    if (threaded) return;
    REQUIRE(t.bin_slots.size() <= Tab::kMaxBinSlots, "I6", "more slots than kMaxBinSlots");
    size_t blocks = 0;
    for (auto& sl : t.bin_slots) blocks += sl.scratch != nullptr;
    REQUIRE((long)blocks == m.live_blocks, "I6", "the table and the runtime disagree about the blocks that exist");
  }
  // destroying the handle; returns whether the device was synchronised for it
  bool destroy() {
    const long syncs0 = m.device_syncs;
    scratch_slots::destroy_wait(t, [] { return true; });
    REQUIRE(m.all_uses_complete(), "I5", "the wait at destroy returned with a use still in flight");
    const bool synced = m.device_syncs != syncs0;
    scratch_slots::free_blocks(t, [](Slot&) {});
    REQUIRE(m.allocs == m.frees, "I6", "blocks allocated and blocks freed differ at destroy");
    REQUIRE(m.events_created == m.events_destroyed, "I6", "events created and events destroyed differ at destroy");
    return synced;
  }
};

#define EXPECT(cond) REQUIRE(cond, "SCENARIO", #cond)

// ---------------------------------------------------------------------------------------------------------------
// Scenarios.
static void s_same_stream() {  // step 1
  World w;
  const MStream a = w.m.create(1);
  auto r = w.launch(a, 100, true);
  EXPECT(r.slot == 0 && w.m.allocs == 1);
  for (int k = 0; k < 5; ++k) {
    r = w.launch(a, 100, k % 2 == 0);
    EXPECT(r.slot == 0 && r.commands == 0 && r.event_calls == 0);
  }
  EXPECT(w.m.allocs == 1 && w.m.commands == 0);
  EXPECT(!w.destroy());
}

static void s_idle_block() {  // step 2: the event complete / not complete
  World w;
  const MStream a = w.m.create(1), b = w.m.create(2), c = w.m.create(3);
  w.launch(a, 100, true);
  auto r = w.launch(b, 100, true);  // a's use is in flight: its event is recorded now, reads pending -> step 3
  EXPECT(r.slot == 1 && w.m.commands == 1 && w.t.bin_slots[0].recorded);
  r = w.launch(c, 100, false);      // nothing complete, nothing may be made: step 4 waits for the older block
  EXPECT(r.slot == 0 && r.commands == 2);  // (b's record, c's wait)
  w.m.advance(0, 100);
  w.m.advance(1, 100);
  w.m.advance(2, 100);
  r = w.launch(a, 100, false);      // b's block: its event reads complete -> step 2, nothing to wait for on the device
  EXPECT(r.slot == 1 && w.m.allocs == 2);
  EXPECT(!w.destroy());
}

static void fill(World& w, MStream* s, int n, size_t bytes) {
  for (int k = 0; k < n; ++k) {
    s[k] = w.m.create(k + 1);
    auto r = w.launch(s[k], bytes, true);
    EXPECT(r.slot == k);
  }
}

static void s_new_block() {  // step 3, up to the table's size and not beyond
  World w;
  MStream s[5];
  fill(w, s, 4, 100);
  EXPECT(w.m.allocs == 4 && w.t.bin_slots.size() == 4);
  s[4] = w.m.create(5);
  auto r = w.launch(s[4], 100, true);
  EXPECT(r.slot == 0 && w.m.allocs == 4);
  EXPECT(!w.destroy());
}

static void s_lru_waited() {  // step 4
  World w;
  MStream s[6];
  fill(w, s, 4, 100);
  s[4] = w.m.create(5);
  s[5] = w.m.create(6);
  const long c0 = w.m.commands;
  auto r = w.launch(s[4], 100, true);
  EXPECT(r.slot == 0 && w.m.commands == c0 + 2);  // the fourth block's record, this stream's wait
  r = w.launch(s[5], 100, false);
  EXPECT(r.slot == 1 && r.commands == 2);  // slot 0's record behind s[4], this stream's wait for slot 1
  EXPECT(w.m.allocs == 4 && w.m.frees == 0);
  EXPECT(!w.destroy());
}

static void s_growth() {  // step 5: the table full and every block too small
  World w;
  MStream s[5];
  fill(w, s, 4, 100);
  s[4] = w.m.create(5);
  auto r = w.launch(s[4], 1000, false);
  EXPECT(r.slot == -1 && r.why == INTERPN_HIP_WHY_NO_SCRATCH && w.m.allocs == 4);
  r = w.launch(s[4], 1000, true);
  EXPECT(r.slot == 0 && w.m.allocs == 5 && w.m.frees == 1 && w.t.bin_slots[0].bytes == 1000);
  r = w.launch(s[0], 100, false);  // the stream that used the old block: the new one is another allocation, and idle blocks come first
  EXPECT(r.slot != -1);
  EXPECT(!w.destroy());
}

static void s_reserve_in_flight() {  // the reserve routine growing a block whose use is in flight
  World w;
  const MStream a = w.m.create(1);
  w.launch(a, 100, true);
  EXPECT(w.reserve(1000, 1) == INTERPN_HIP_OK);
  EXPECT(w.m.allocs == 2 && w.m.frees == 1 && w.m.all_uses_complete());
  EXPECT(w.reserve(1000, 3) == INTERPN_HIP_OK && w.m.allocs == 4 && w.t.bin_slots.size() == 3);
  EXPECT(w.reserve(1000, 3) == INTERPN_HIP_OK && w.m.allocs == 4);
  EXPECT(w.reserve(2000, 4) == INTERPN_HIP_OK && w.t.bin_slots.size() == 4 && w.m.live_blocks == 4);
  auto r = w.launch(a, 2000, false);
  EXPECT(r.slot != -1);
  EXPECT(!w.destroy());
}

static void s_capture() {
  World w;
  const MStream a = w.m.create(1), b = w.m.create(2);
  w.launch(a, 100, true);
  w.m.set_capture(a, true);
  auto r = w.launch(b, 100, false);  // the only block's last stream is being captured: nobody else gets it
  EXPECT(r.slot == -1 && r.why == INTERPN_HIP_WHY_NO_SCRATCH && w.m.commands == 0);
  EXPECT(w.reserve(1000, 1) == INTERPN_HIP_OK && w.m.frees == 0 && w.t.bin_slots.size() == 2);  // ... nor is it regrown
  r = w.launch(a, 100, false);       // the capturing stream itself: a block without any runtime call
  EXPECT(r.slot == 0 && r.commands == 0 && r.event_calls == 0);
  EXPECT(w.t.sync_device_at_destroy);  // (the captured launch cannot be marked)
  w.m.set_capture(a, false);
  r = w.launch(b, 100, false);
  EXPECT(r.slot == 1);  // (the block reserve added: never used, so it comes first)
  r = w.launch(w.m.create(3), 100, false);
  EXPECT(r.slot == 0 && r.commands == 2);  // capture over: a's block was settled by b's launch and can be waited for again (b's record, the wait)
  EXPECT(w.destroy());
  World v;  // a marked stream that is being captured when the handle is destroyed
  const MStream c = v.m.create(1);
  v.launch(c, 100, true);
  v.m.set_capture(c, true);
  EXPECT(!v.t.sync_device_at_destroy && v.destroy());
}

static void s_destroyed_stream() {  // I7
  for (int answers = 0; answers < 2; ++answers) {  // the capture query of the dead stream fails / succeeds, and then the record fails
    World w;
    w.m.dead_stream_answers_query = answers != 0;
    const MStream a = w.m.create(1), b = w.m.create(2);
    w.launch(a, 100, true);
    w.m.destroy_stream(a);
    auto r = w.launch(b, 100, false);  // no event can be recorded behind a's use: the device is waited for instead
    EXPECT(r.slot == 0 && w.m.device_syncs == 1 && w.t.sync_device_at_destroy && r.commands == 0);
    EXPECT(w.destroy() && w.m.device_syncs == 2);
  }
}

static void s_alloc_failure() {
  World w;
  MStream s[5];
  s[0] = w.m.create(1);
  w.m.fail_alloc_in = 1;  // step 3
  auto r = w.launch(s[0], 100, true);
  EXPECT(r.slot == -1 && r.why == INTERPN_HIP_WHY_ALLOC_FAILED && w.m.events_created == 1 && w.m.events_destroyed == 1);
  w.m.fail_event_in = 1;
  r = w.launch(s[0], 100, true);
  EXPECT(r.slot == -1 && r.why == INTERPN_HIP_WHY_ALLOC_FAILED && w.t.bin_slots.empty());
  r = w.launch(s[0], 100, true);
  EXPECT(r.slot == 0);
  for (int k = 1; k < 4; ++k) {
    s[k] = w.m.create(k + 1);
    w.launch(s[k], 100, true);
  }
  s[4] = w.m.create(5);
  w.m.fail_alloc_in = 1;  // step 5: the old block is gone, the new one did not come
  r = w.launch(s[4], 1000, true);
  EXPECT(r.slot == -1 && r.why == INTERPN_HIP_WHY_ALLOC_FAILED && w.m.live_blocks == 3 && w.t.bin_slots[0].bytes == 0);
  r = w.launch(s[0], 100, false);  // the table goes on
  EXPECT(r.slot != -1 && r.slot != 0);
  r = w.launch(s[4], 1000, true);
  EXPECT(r.slot == 0 && w.m.live_blocks == 4);
  w.m.fail_alloc_in = 1;  // the reserve routine
  EXPECT(w.reserve(5000, 1) == INTERPN_HIP_ERR_OUT_OF_MEMORY);
  EXPECT(w.reserve(5000, 1) == INTERPN_HIP_OK);
  w.m.fail_event_in = 1;
  World v;
  v.m.fail_event_in = 1;
  EXPECT(v.reserve(100, 1) == -1 && v.reserve(100, 2) == INTERPN_HIP_OK);
  EXPECT(!v.destroy());
  EXPECT(!w.destroy());
}

static void s_destroy_wait() {  // I5
  World w;
  MStream s[17];
  for (int k = 0; k < 16; ++k) {
    s[k] = w.m.create(k + 1);
    w.launch(s[k], 100, true);
    w.launch(s[k], 100, true);
  }
  EXPECT(w.t.marks.size() == 16 && !w.t.sync_device_at_destroy);
  EXPECT(!w.destroy() && w.m.device_syncs == 0);  // sixteen live streams: each waited for, the device never
  World v;
  for (int k = 0; k < 17; ++k) {
    s[k] = v.m.create(k + 1);
    v.launch(s[k], 100, true);
  }
  EXPECT(v.t.marks.size() == 16 && v.t.sync_device_at_destroy);
  EXPECT(v.destroy());  // the seventeenth could not be noted
  World u;
  s[0] = u.m.create(1);
  s[1] = u.m.create(2);
  u.launch(s[0], 100, true);
  u.launch(s[1], 100, true);
  u.m.destroy_stream(s[1]);
  EXPECT(!u.t.sync_device_at_destroy && u.destroy());  // a noted stream that is gone
}

static void s_stream_value_reused() {
  {
    World w;
    const MStream a = w.m.create(1);
    w.launch(a, 100, true);
    w.m.host_sync(a);  // the caller's part
    w.m.destroy_stream(a);
    const MStream again = w.m.create(1);  // the runtime hands the same value out
    auto r = w.launch(again, 100, false);
    EXPECT(r.slot == 0 && r.commands == 0 && r.event_calls == 0);
    EXPECT(!w.destroy());
  }
  {
    World w;
    const MStream a = w.m.create(1);
    w.launch(a, 100, true);
    w.m.destroy_stream(a);
    const MStream again = w.m.create(1);
    g_expect = "I1";  // not covered by the library: step 1 sees "the same stream", and the old use may still be running
    g_expected_seen = false;
    w.launch(again, 100, false);
    g_expect.clear();
    EXPECT(g_expected_seen);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Seeded random walk.
static long walk(unsigned seed, long ops) {
  g_seed = seed;
  std::mt19937 rng(seed);
  auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
  static const size_t kNeeds[] = {64, 64, 128, 128, 256, 512, 1024, 4096};
  long launches = 0, handles = 0;
  long op = 0;
  while (op < ops) {
    World w;
    ++handles;
    int next_value = 1;
    std::vector<MStream> s;
    for (int k = 0; k < 6; ++k) s.push_back(w.m.create(next_value++));
    const long life = 500 + pick(2500);
    for (long k = 0; k < life && op < ops; ++k, ++op) {
      g_op = op;
      const int what = pick(100);
      if (what < 55) {
        w.launch(s[pick(6)], kNeeds[pick(8)], pick(10) < 7);
        ++launches;
      } else if (what < 60) {
        w.reserve(kNeeds[pick(8)], 1 + pick(4));
      } else if (what < 80) {
        w.m.advance(pick((int)w.m.gens.size()), 1 + pick(5));
      } else if (what < 85) {
        const MStream x = s[pick(6)];
        w.m.set_capture(x, !w.m.capturing(x));
      } else if (what < 87) {
        const int i = pick(6);
        w.m.destroy_stream(s[i]);
        s[i] = w.m.create(next_value++);  // (a fresh value: see the scenario stream_value_reused)
      } else if (what < 91) {
        (pick(3) ? w.m.fail_alloc_in : w.m.fail_event_in) = 1 + pick(2);
      } else if (what < 96) {
        w.m.host_sync(s[pick(6)]);
      } else {
        w.m.advance(pick((int)w.m.gens.size()), 1000);
      }
    }
    w.m.fail_alloc_in = w.m.fail_event_in = 0;
    w.destroy();
  }
  std::printf("walk seed %u operations %ld launches %ld handles %ld\n", seed, op, launches, handles);
  return op;
}

// ---------------------------------------------------------------------------------------------------------------
// Four host threads through one table (the lock that step 5 drops around its wait).
static void threads() {
  g_scenario = "threads";
  World w;
  w.threaded = true;
  std::vector<MStream> s;
  for (int k = 0; k < 8; ++k) s.push_back(w.m.create(k + 1));
  std::vector<std::thread> pool;
  for (int th = 0; th < 4; ++th)
    pool.emplace_back([&w, &s, th] {
      std::mt19937 rng(1000u + (unsigned)th);
      for (int k = 0; k < 2000; ++k) {
        const MStream mine = s[2 * th + (int)(rng() % 2u)];
        const size_t need = rng() % 3u ? (size_t)64 * (size_t)(1 + k / 10) : 64;  // needs keep outgrowing the blocks: step 5, again and again
        w.launch(mine, need, rng() % 10u < 8u);
        if (rng() % 4u == 0) {
          std::lock_guard<std::mutex> lk(w.m.mu);
          w.m.advance((int)(rng() % 8u), 1 + (int)(rng() % 4u));
        }
      }
    });
  for (auto& th : pool) th.join();
  w.threaded = false;
  w.check();
  w.destroy();
  std::printf("threads uses %ld allocs %ld frees %ld\n", w.m.uses, w.m.allocs, w.m.frees);
  REQUIRE(w.m.uses > 4000 && w.m.allocs > 40, "TEST", "the threads did not get to grow blocks");
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "threads")) {
    threads();
    return 0;
  }
  struct { const char* name; void (*run)(); } scenarios[] = {
      {"same_stream", s_same_stream},       {"idle_block", s_idle_block},
      {"new_block", s_new_block},           {"lru_waited", s_lru_waited},
      {"growth", s_growth},                 {"reserve_in_flight", s_reserve_in_flight},
      {"capture", s_capture},               {"destroyed_stream", s_destroyed_stream},
      {"alloc_failure", s_alloc_failure},   {"destroy_wait", s_destroy_wait},
      {"stream_value_reused", s_stream_value_reused}};
  for (auto& sc : scenarios) {
    g_scenario = sc.name;
    sc.run();
    std::printf("scenario %s ok\n", sc.name);
  }
  if (argc > 1 && !std::strcmp(argv[1], "scenarios")) return 0;
  g_scenario = "walk";
  for (unsigned seed : {20260101u, 7u, 4242u})
    if (walk(seed, 20000) < 20000) return 1;
  return 0;
}
"""

SCENARIOS = ["same_stream", "idle_block", "new_block", "lru_waited", "growth", "reserve_in_flight", "capture",
             "destroyed_stream", "alloc_failure", "destroy_wait", "stream_value_reused"]


def _build(tmp, name, flags):
    src = tmp / "scratch_slots_model.cpp"
    src.write_text(PROGRAM)
    exe = tmp / name
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Wextra", "-pthread", *flags, "-I", CSRC,
                           str(src), "-o", str(exe)])
    return exe


needs_cxx = pytest.mark.skipif(shutil.which(CXX) is None, reason="needs g++")


@needs_cxx
def test_header_has_no_hip_in_it_and_compiles_alone(tmp_path):
    text = open(HEADER).read()
    assert "#include <hip" not in text and "hip_runtime" not in text
    src = tmp_path / "alone.cpp"
    src.write_text('#include "scratch_slots.h"\nint main() { return 0; }\n')
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-c", str(src), "-o", str(tmp_path / "alone.o")])


@needs_cxx
def test_scenarios_and_random_walk_keep_the_invariants(tmp_path):
    exe = _build(tmp_path, "model", ["-O1", "-Werror"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for name in SCENARIOS:
        assert "scenario %s ok" % name in out.stdout
    walks = [line.split() for line in out.stdout.splitlines() if line.startswith("walk ")]
    assert len(walks) == 3 and len({w[2] for w in walks}) == 3
    for w in walks:
        assert int(w[4]) >= 20000 and int(w[6]) > 8000 and int(w[8]) >= 8, w


@needs_cxx
@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_four_threads_through_one_table(tmp_path, sanitizer):
    """A stand-alone program, run directly: the sanitizer's runtime is linked into it."""
    exe = _build(tmp_path, "model_threads", ["-O1", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all"])
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    out = subprocess.run([str(exe), "threads"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "threads uses" in out.stdout and "VIOLATION" not in out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]


MUTANTS = {
    "a_take_without_the_stream_wait": (
        "    const int e = t.rt.stream_wait_event(stream, pick->event);\n", "    const int e = 0;\n", ("I1",)),
    "b_settle_clears_unmarked_without_recording": (
        "  if (e == 0) e = t.rt.event_record(sl.event, sl.last_stream);\n", "\n", ("I1", "I2")),
    "c_step_1_for_any_stream": (
        "    if (sl.last_stream == stream) { pick = &sl; break; }\n", "    { pick = &sl; break; }\n", ("I1",)),
    "d_release_does_not_set_unmarked": (
        "  slot->unmarked = true;\n", "\n", ("I1",)),
    "e_growth_frees_without_the_event_synchronise": (
        "      bool ok = !recorded || t.rt.event_synchronize(ev) == 0;\n", "      bool ok = true;\n", ("I2",)),
    "f_destroy_wait_skips_the_stream_synchronise": (
        "      if (e == 0 && !capturing) e = t.rt.stream_synchronize(m);\n", "\n", ("I5",)),
    "g_settle_ignores_the_capture_state": (
        "  if (e == 0 && capturing) return false;\n", "\n", ("I3",)),
}


@needs_cxx
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_model_rejects_a_mutated_header(tmp_path, mutant):
    line, replacement, must_violate = MUTANTS[mutant]
    text = open(HEADER).read()
    assert text.count(line) == 1, (mutant, text.count(line))
    # the copy sits where the header's relative include of the C ABI's status codes (../../include) still resolves
    csrc = tmp_path / "pkg" / "csrc"
    os.makedirs(csrc)
    (csrc / "scratch_slots.h").write_text(text.replace(line, replacement))
    os.makedirs(tmp_path / "include")
    shutil.copy(os.path.join(ROOT, "include", "interpn_hip.h"), tmp_path / "include" / "interpn_hip.h")
    src = tmp_path / "scratch_slots_model.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "mutant"
    subprocess.check_call([CXX, "-std=c++17", "-O0", "-w", "-pthread", "-I", str(csrc), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), "scenarios"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0, (mutant, out.stdout[-1000:])
    assert any("VIOLATION %s:" % inv in out.stdout for inv in must_violate), (mutant, out.stdout[-1000:])
