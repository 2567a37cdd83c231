// many_shape.hpp -- which climbs of one round of mpf_optimize_spr_many_round form the launch of k_climb_many, on what shape, and
// which run alone.  Host only, no device header: Engine::climb_many_round (climb_host.cpp) fills the table and acts on the
// answer, many_shape_main.cpp drives the same function over a table of cases (tests/test_many_shape_host.py).
//
// A launch of k_climb_many has ONE shape for all its workgroups: the tile width (16 x vw words), the number of states, the
// word-major flag and the device.  A climb is laid out for a shape when it starts (tiles, the per-tile scores, its ClimbParams
// follow from the width; the width follows from the row pitch, which follows from the weights) and keeps it until it is done:
//   - climbs that CONTINUE give the shape.  Two of them that disagree cannot share a launch: MPF_E_STATE.
//   - a continuing climb whose engine was packed again since it started (set_weights between two rounds), or whose fitted shape
//     is no longer the one it started on (an option changed), is laid out for rows that no longer exist: MPF_E_STATE.
//   - a STARTING climb whose own shape is not the launch's runs alone (mpf_optimize_spr), as every engine the batch cannot take.
//   - where no climb continues, the first starting climb that fits the batch gives the shape.
// Nothing is touched before the decision is made: an error leaves every engine as it was.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mpfitch.h"

namespace mpf {

struct ManyShape {
  int vw = 0, S = 0, dev = 0;                    // words per lane group (0 = no width fits), states, device
  bool wm = false;                               // four-state data a word per lane (64-word tiles)
  bool operator==(const ManyShape &o) const { return vw == o.vw && S == o.S && dev == o.dev && wm == o.wm; }
  bool operator!=(const ManyShape &o) const { return !(*this == o); }
};

struct ManyEntry {
  uint8_t state = 0;                             // 0 = takes no part, 1 = a climb starts, 2 = its climb goes on
  ManyShape now;                                 // what the engine's packing and options fit at this moment
  uint64_t pack_gen = 0;                         // the engine's packing generation at this moment
  bool fits = false;                             // state 1: the batch can take this engine at all (no tracker, not weighted, ...)
  ManyShape started;                             // state 2: the shape its climb started on ...
  uint64_t started_gen = 0;                      // ... and the packing generation then (0 = no climb was started)
};

struct ManyPlan {
  int rc = MPF_OK;
  std::string error;
  ManyShape shape;                               // valid where batch is not empty
  std::vector<int> batch;                        // indices of the launch's climbs, ascending; batch[0] owns the parameter blocks and the stream
  std::vector<int> alone;                        // starting climbs that run by themselves, ascending
};

inline std::string many_shape_text(const ManyShape &s)
{
  return std::to_string(16 * s.vw) + "-word tiles, " + std::to_string(s.S) + " states" + (s.wm ? ", word-major" : "") + ", device " + std::to_string(s.dev);
}

inline ManyPlan many_shape_decide(const ManyEntry *e, int n)
{
  ManyPlan p;
  int lead = -1;                                 // the first continuing climb
  for (int k = 0; k < n; k++) {
    if (e[k].state != 2) continue;
    if (e[k].started_gen == 0 || e[k].started.vw <= 0) {
      p.rc = MPF_E_STATE;
      p.error = "mpf_optimize_spr_many_round: engine " + std::to_string(k) + " is to continue a climb that was never started";
      return p;
    }
    if (e[k].pack_gen != e[k].started_gen) {
      p.rc = MPF_E_STATE;
      p.error = "mpf_optimize_spr_many_round: engine " + std::to_string(k) + " was packed again (weights changed) in the middle of its climb";
      return p;
    }
    if (e[k].now != e[k].started) {
      p.rc = MPF_E_STATE;
      p.error = "mpf_optimize_spr_many_round: engine " + std::to_string(k) + " started its climb on " + many_shape_text(e[k].started) +
                " and now fits " + many_shape_text(e[k].now) + " (an option changed in the middle of the climb)";
      return p;
    }
    if (lead < 0) { lead = k; p.shape = e[k].started; continue; }
    if (e[k].started != p.shape) {
      p.rc = MPF_E_STATE;
      p.error = "mpf_optimize_spr_many_round: the climbs of engines " + std::to_string(lead) + " and " + std::to_string(k) + " go on in different shapes (" +
                many_shape_text(p.shape) + " / " + many_shape_text(e[k].started) + "): they cannot share a launch";
      return p;
    }
  }
  bool have = lead >= 0;
  if (!have)
    for (int k = 0; k < n && !have; k++)
      if (e[k].state == 1 && e[k].fits && e[k].now.vw > 0) { p.shape = e[k].now; have = true; }
  for (int k = 0; k < n; k++) {
    if (e[k].state == 2) p.batch.push_back(k);
    else if (e[k].state == 1) {
      if (have && e[k].fits && e[k].now == p.shape) p.batch.push_back(k);
      else p.alone.push_back(k);
    }
  }
  return p;
}

}  // namespace mpf
