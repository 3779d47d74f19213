// The validity rule of recorded merge plans (csrc/replay_rule.h), stand-alone under ASan + UBSan
// (tests/test_replay_rule_host.py). Prints "ok <checks>" and exits 0, or the failed check and 1.
#include <cstdio>

#include "../../approximated_personalized_pagerank_amd/csrc/replay_rule.h"

static int checks = 0, bad = 0;
#define CHECK_EQ(expr, want)                                                                  \
  do {                                                                                        \
    const long long got_ = (long long)(expr), want_ = (long long)(want);                      \
    checks++;                                                                                 \
    if (got_ != want_) {                                                                      \
      bad++;                                                                                  \
      std::fprintf(stderr, "%s:%d: %s = %lld, want %lld\n", __FILE__, __LINE__, #expr, got_, want_); \
    }                                                                                         \
  } while (0)

// the clock after an update's closing read of the device counter
static ReplayClock read(ReplayClock c, uint64_t counter) {
  c.len_changes = counter;
  c.valid = true;
  return c;
}

int main() {
  const ReplayKnobs on;
  CHECK_EQ(replay_allowed(on), 1);
  ReplayClock c;
  // nothing was read yet: a plan stamped now is not live, and nothing replays
  CHECK_EQ(replay_stamp(c, 0, 0, 100).live, 0);
  CHECK_EQ(replay_valid(replay_stamp(c, 0, 0, 100), c, 0, 0, 100, on), 0);
  // the init's merge ends with a read; update 0 of partition 0 records, update 1 of partition 1 too
  c = read(c, 0);
  const ReplayStamp s0 = replay_stamp(c, 0, 0, 100);
  CHECK_EQ(s0.live, 1);
  c = read(c, 37);  // update 0 changed 37 lengths
  const ReplayStamp s1 = replay_stamp(c, 1, 0, 80);
  c = read(c, 37);  // update 1 changed none
  // update 2: the counter moved since s0 was stamped
  CHECK_EQ(replay_valid(s0, c, 0, 0, 100, on), 0);
  const ReplayStamp s2 = replay_stamp(c, 0, 0, 100);
  c = read(c, 37);
  // update 3: unchanged since s1 was stamped -> replays
  CHECK_EQ(replay_valid(s1, c, 1, 0, 80, on), 1);
  c = read(c, 37);
  // update 4: unchanged since s2 -> replays; and again at 6 from the same stamp
  CHECK_EQ(replay_valid(s2, c, 0, 0, 100, on), 1);
  c = read(c, 37);
  c = read(c, 37);
  CHECK_EQ(replay_valid(s2, c, 0, 0, 100, on), 1);
  // one more changed length, in either partition's update, ends it
  const ReplayClock moved = read(c, 38);
  CHECK_EQ(replay_valid(s2, moved, 0, 0, 100, on), 0);
  CHECK_EQ(replay_valid(s1, moved, 1, 0, 80, on), 0);
  // (a counter reset to an equal-looking value by a new run comes with a drop: see below)
  // another list range, or the other partition's list
  CHECK_EQ(replay_valid(s2, c, 0, 0, 50, on), 0);
  CHECK_EQ(replay_valid(s2, c, 0, 50, 100, on), 0);
  CHECK_EQ(replay_valid(s2, c, 0, 1, 100, on), 0);
  CHECK_EQ(replay_valid(s2, c, 0, 0, 101, on), 0);
  CHECK_EQ(replay_valid(s2, c, 1, 0, 100, on), 0);
  // an init in between: the drop invalidates every stamp, even once the counter reads the same again
  ReplayClock d = c;
  replay_drop(d);
  CHECK_EQ(d.valid, 0);
  CHECK_EQ(replay_valid(s2, d, 0, 0, 100, on), 0);
  d = read(d, 37);
  CHECK_EQ(replay_valid(s2, d, 0, 0, 100, on), 0);
  CHECK_EQ(replay_valid(s1, d, 1, 0, 80, on), 0);
  // ... and plans stamped after it replay among themselves
  const ReplayStamp s3 = replay_stamp(d, 0, 0, 100);
  d = read(d, 37);
  d = read(d, 37);
  CHECK_EQ(replay_valid(s3, d, 0, 0, 100, on), 1);
  // a stamp that is not live never replays
  ReplayStamp dead = s3;
  dead.live = false;
  CHECK_EQ(replay_valid(dead, d, 0, 0, 100, on), 0);
  // each disabling knob
  ReplayKnobs k;
  k.enabled = false;
  CHECK_EQ(replay_allowed(k), 0);
  CHECK_EQ(replay_valid(s3, d, 0, 0, 100, k), 0);
  k = ReplayKnobs{};
  k.sharded = true;
  CHECK_EQ(replay_allowed(k), 0);
  CHECK_EQ(replay_valid(s3, d, 0, 0, 100, k), 0);
  k = ReplayKnobs{};
  k.wave_by_d = true;
  CHECK_EQ(replay_allowed(k), 0);
  CHECK_EQ(replay_valid(s3, d, 0, 0, 100, k), 0);
  k = ReplayKnobs{};
  k.sv_seedless = true;
  CHECK_EQ(replay_allowed(k), 0);
  CHECK_EQ(replay_valid(s3, d, 0, 0, 100, k), 0);
  k = ReplayKnobs{};
  k.hot = true;
  CHECK_EQ(replay_allowed(k), 0);
  CHECK_EQ(replay_valid(s3, d, 0, 0, 100, k), 0);
  CHECK_EQ(replay_valid(s3, d, 0, 0, 100, ReplayKnobs{}), 1);
  // the order of the updates: iteration after iteration, each over its whole list (100 / 80 sources)
  ReplayClock o = read(ReplayClock{}, 5);
  replay_begin_update(o, 0, 100, 80, true);
  CHECK_EQ(o.valid, 1);
  CHECK_EQ(o.last_it, 0);
  const ReplayStamp t0 = replay_stamp(o, 0, 0, 100);
  const uint64_t e0 = o.epoch;
  replay_begin_update(o, 1, 80, 100, true);
  const ReplayStamp t1 = replay_stamp(o, 1, 0, 80);
  replay_begin_update(o, 2, 100, 80, true);
  CHECK_EQ(o.epoch, e0);
  CHECK_EQ(replay_valid(t0, o, 0, 0, 100, on), 1);
  // iteration 3 in two half ranges: both belong to it, and iteration 4 follows a covered list
  replay_begin_update(o, 3, 40, 100, true);
  CHECK_EQ(replay_valid(t1, o, 1, 0, 40, on), 0);  // (a half is another range)
  replay_begin_update(o, 3, 40, 100, true);
  CHECK_EQ(o.covered, 80);
  replay_begin_update(o, 4, 100, 80, true);
  CHECK_EQ(o.epoch, e0);
  CHECK_EQ(replay_valid(t0, o, 0, 0, 100, on), 1);
  // iteration 5 covers only half of its list: iteration 6 reads rows no counted update replaced
  replay_begin_update(o, 5, 40, 100, true);
  replay_begin_update(o, 6, 100, 80, true);
  CHECK_EQ(o.epoch, e0 + 1);
  CHECK_EQ(replay_valid(t0, o, 0, 0, 100, on), 0);
  CHECK_EQ(o.valid, 1);  // (the counter is still good: a plan stamped now starts a new chain)
  const ReplayStamp t6 = replay_stamp(o, 0, 0, 100);
  replay_begin_update(o, 7, 80, 100, true);
  replay_begin_update(o, 8, 100, 80, true);
  CHECK_EQ(replay_valid(t6, o, 0, 0, 100, on), 1);
  // a skipped iteration, a repeated earlier one, and a list that is not the partition's own
  ReplayClock q = o;
  replay_begin_update(q, 10, 100, 80, true);
  CHECK_EQ(replay_valid(t6, q, 0, 0, 100, on), 0);
  q = o;
  replay_begin_update(q, 6, 100, 80, true);
  CHECK_EQ(replay_valid(t6, q, 0, 0, 100, on), 0);
  q = o;
  replay_begin_update(q, 9, 80, 100, false);
  CHECK_EQ(q.valid, 0);
  CHECK_EQ(replay_valid(t6, q, 0, 0, 100, on), 0);
  if (bad) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
