// When a recorded merge plan may be replayed. Pure host code, no HIP: the rule is
// compiled alone and run under the sanitizers by tests/test_replay_rule_host.py.
//
// An exact-sum GRank update plans from row lengths only: a source's candidate count is the sum of
// its successors' row lengths, its tier follows from that count, and the sieve / range split from
// the count and from whether its own row is full. The merge kernels count every row they store
// with a length other than the one it replaces (ppr_common.h finish_source, PPR_STAT_LENCHG). While
// that count stands still, the plan of (partition, list range) recorded two updates earlier is the
// plan a fresh classification would produce, and every buffer it sized is still large enough.
#pragma once
#include <cstdint>

// what makes the classification depend on more than row lengths, or the rows arrive from elsewhere
struct ReplayKnobs {
  bool enabled = true;       // PPR_REPLAY
  bool sharded = false;      // the plan has a communicator / ran a sharded loop: rows arrive by exchange
  bool wave_by_d = false;    // PPR_WAVE_BY_D=1: wave tiers by the last distinct-key count
  bool sv_seedless = false;  // PPR_SV_SEEDLESS=1: the sieve split follows the retry-grid history
  bool hot = false;          // a hot key set is configured (PPR_HOT_N): the sieve is off once it is built
};
inline bool replay_allowed(const ReplayKnobs& k) {
  return k.enabled && !k.sharded && !k.wave_by_d && !k.sv_seedless && !k.hot;
}

// the plan's view of the device counter: the value read at the end of the last update (`valid`:
// one has been read since the cache was last dropped) and the drop count (ppr_grank_plan_init, a row
// import, an MC run: everything that writes row lengths without counting). The counter speaks for
// the rows an update reads only while the updates come as the job's loop issues them -- iteration
// after iteration, each over its whole list: then the rows update `it` reads are those updates
// it - 1 and it - 2 wrote over the ones the recorded plan read. `last_it` / `covered` follow that.
struct ReplayClock {
  uint64_t len_changes = 0;
  uint64_t epoch = 0;
  bool valid = false;
  int last_it = -1;     // iteration of the last update (-1: none since the init)
  int64_t covered = 0;  // sources its calls covered so far
};

// taken just before a recorded plan's classification ran
struct ReplayStamp {
  bool live = false;
  int part = -1;
  int64_t begin = 0, end = 0;  // the range of the partition's active list the plan covers
  uint64_t len_changes = 0;
  uint64_t epoch = 0;
};

inline ReplayStamp replay_stamp(const ReplayClock& c, int part, int64_t begin, int64_t end) {
  ReplayStamp s;
  s.live = c.valid;
  s.part = part;
  s.begin = begin;
  s.end = end;
  s.len_changes = c.len_changes;
  s.epoch = c.epoch;
  return s;
}

// may the plan stamped `s` stand in for a fresh classification of [begin, end) of `part` now?
inline bool replay_valid(const ReplayStamp& s, const ReplayClock& now, int part, int64_t begin, int64_t end,
                         const ReplayKnobs& k) {
  return replay_allowed(k) && s.live && now.valid && s.epoch == now.epoch && s.part == part && s.begin == begin &&
         s.end == end && s.len_changes == now.len_changes;
}

inline void replay_drop(ReplayClock& c) {
  c.epoch++;
  c.valid = false;
  c.last_it = -1;
  c.covered = 0;
}

// An update call of iteration `it` over `count` sources begins; `prev_list` is the length of the
// list the previous iteration had to cover. Further ranges of the same iteration add up; anything
// but the next iteration after a fully covered one (iteration 0 after an init) drops the cache: some
// row may then be read that no counted update wrote over the one a recorded plan saw.
// `in_list`: the call updates a range of its partition's own active list.
inline void replay_begin_update(ReplayClock& c, int it, int64_t count, int64_t prev_list, bool in_list) {
  if (in_list && it == c.last_it) {
    c.covered += count;
    return;
  }
  const bool next = in_list && it == c.last_it + 1 && (c.last_it < 0 || c.covered == prev_list);
  if (!next) {
    const bool was_valid = c.valid;
    replay_drop(c);
    // (the counter itself is still good: plans stamped from here on start a new chain)
    c.valid = was_valid && in_list;
  }
  c.last_it = it;
  c.covered = count;
}
