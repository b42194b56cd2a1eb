// The tracker's host twin (csrc/track_twin.h over csrc/track_rule.h) under the address and undefined-behaviour sanitizers, as a
// stand-alone host program: no Python, no GPU; host-only work, not for a machine with a GPU.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Ifacerecognition-multiarchitecture-pipeline_amd/csrc tools/track_twin_check.cpp -o /tmp/track_twin_check && /tmp/track_twin_check < cases.txt
//
// It reads sequences from standard input, steps the twin through them in buffers of EXACTLY the sizes the ABI states (so a read
// or write one element outside is a sanitizer report) and prints every step's ids, crops and state; tests/test_track_cpu.py
// feeds it the hand-built sequences and the size grid and compares the output with frames.track_boxes.  Without input it runs
// two small sequences of its own (IoU exactly at the threshold; coordinates beyond 2^31) and checks them itself.
//
// Input, whitespace separated; floats as the 8 hex digits of their bits (NaN and infinities pass unchanged):
//   sequence:  "seq" n_streams max_boxes n_steps has_probs det_thresh iou_thresh
//   per step:  per stream: n H W, then n times x1 y1 x2 y2 [prob]
//   rejection: "reject" n_streams max_boxes count0      a call that must be refused, with the state left untouched
// Output per step and stream: "ids" n ids..., "rois" 4 n ints..., "state" P next_id, P times (4 floats as hex, id).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "track_twin.h"

static float hex_float(const std::string& h) {
  const uint32_t u = (uint32_t)strtoul(h.c_str(), nullptr, 16);
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t float_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static bool word(std::string& w) {
  char buf[64];
  if (scanf("%63s", buf) != 1) return false;
  w = buf;
  return true;
}
static std::string need() {
  std::string w;
  if (!word(w)) { fprintf(stderr, "track_twin_check: input ends inside a record\n"); exit(2); }
  return w;
}

struct Run {                                     // buffers of exactly the stated sizes, on the heap
  int S, M;
  std::vector<unsigned char> state;
  std::vector<float> boxes, probs;
  std::vector<int32_t> counts, hw, ids, rois;
  Run(int S_, int M_) : S(S_), M(M_), state(frmap_track_bytes(S_, M_), 0), boxes((size_t)S_ * M_ * 4, 7.f), probs((size_t)S_ * M_, 1.f),
                        counts((size_t)S_, 0), hw((size_t)S_ * 2, 0), ids((size_t)S_ * M_, 12345), rois((size_t)S_ * M_ * 4, 12345) {}
  const char* step(bool has_probs, double det, double iou) {
    return frmap_track_step_twin(state.data(), boxes.data(), has_probs ? probs.data() : nullptr, counts.data(), hw.data(), S, M, det,
                                 iou, ids.data(), rois.data());
  }
  void print() const {
    const int32_t* meta = (const int32_t*)state.data();
    const float* sb = (const float*)(state.data() + frmap_track_boxes_offset(S));
    const int32_t* si = (const int32_t*)(state.data() + frmap_track_ids_offset(S, M));
    for (int s = 0; s < S; ++s) {
      printf("ids %d", M);
      for (int i = 0; i < M; ++i) printf(" %d", ids[(size_t)s * M + i]);
      printf("\nrois %d", M);
      for (int i = 0; i < 4 * M; ++i) printf(" %d", rois[(size_t)s * M * 4 + i]);
      printf("\nstate %d %d", meta[2 * s], meta[2 * s + 1]);
      for (int j = 0; j < meta[2 * s]; ++j) {
        for (int c = 0; c < 4; ++c) printf(" %08x", float_bits(sb[((size_t)s * M + j) * 4 + c]));
        printf(" %d", si[(size_t)s * M + j]);
      }
      printf("\n");
    }
  }
};

static int self_check() {
  int bad = 0;
  for (int nudge = 0; nudge < 2; ++nudge) {      // previous (5, 0, 10, 1), current (0, 0, 8, 1): 3 / 10 is not > 0.3; one ulp more is
    Run r(1, 1);
    r.hw = {4, 20};
    r.counts[0] = 1;
    const float prev[4] = {5.f, 0.f, 10.f, 1.f};
    float cur[4] = {0.f, 0.f, 8.f, 1.f};
    if (nudge) cur[2] = nextafterf(8.f, 9.f);
    memcpy(r.boxes.data(), prev, sizeof(prev));
    if (r.step(false, 0.9, 0.3) || r.ids[0] != 0) ++bad;
    memcpy(r.boxes.data(), cur, sizeof(cur));
    if (r.step(false, 0.9, 0.3) || r.ids[0] != (nudge ? 0 : 1)) ++bad;
  }
  {
    Run r(1, 2);
    r.hw = {100, 120};
    r.counts[0] = 2;
    const float b[8] = {-3e9f, -5e9f, 4e9f, 1e10f, 3e9f, 0.f, 4e9f, 10.f};
    memcpy(r.boxes.data(), b, sizeof(b));
    if (r.step(true, 0.9, 0.3) || r.ids[0] != 0 || r.ids[1] != -1 || r.rois[2] != 120 || r.rois[3] != 100) ++bad;
    r.counts[0] = 3;                             // more boxes than slots: refused, nothing written
    const std::vector<unsigned char> before = r.state;
    if (!r.step(true, 0.9, 0.3) || before != r.state) ++bad;
  }
  printf("track_twin_check: self check %s\n", bad ? "FAILED" : "passed");
  return bad ? 1 : 0;
}

int main() {
  std::string w;
  bool any = false;
  while (word(w)) {
    any = true;
    if (w == "seq") {
      const int S = atoi(need().c_str()), M = atoi(need().c_str()), steps = atoi(need().c_str()), has_probs = atoi(need().c_str());
      const double det = atof(need().c_str()), iou = atof(need().c_str());
      if (S < 1 || M < 1 || M > FRMAP_TRACK_MAX_BOXES) { fprintf(stderr, "track_twin_check: bad sequence header\n"); return 2; }
      Run r(S, M);
      printf("seq %d %d %d\n", S, M, steps);
      for (int k = 0; k < steps; ++k) {
        for (int s = 0; s < S; ++s) {
          const int n = atoi(need().c_str());
          if (n < 0 || n > M) { fprintf(stderr, "track_twin_check: count %d of %d\n", n, M); return 2; }
          r.counts[(size_t)s] = n;
          r.hw[2 * (size_t)s] = atoi(need().c_str());
          r.hw[2 * (size_t)s + 1] = atoi(need().c_str());
          for (int i = 0; i < n; ++i) {
            for (int c = 0; c < 4; ++c) r.boxes[((size_t)s * M + i) * 4 + c] = hex_float(need());
            if (has_probs) r.probs[(size_t)s * M + i] = hex_float(need());
          }
        }
        const char* why = r.step(has_probs != 0, det, iou);
        if (why) { fprintf(stderr, "track_twin_check: step refused: %s\n", why); return 3; }
        r.print();
      }
    } else if (w == "reject") {
      const int S = atoi(need().c_str()), M = atoi(need().c_str()), c0 = atoi(need().c_str());
      const int Ma = M >= 1 && M <= FRMAP_TRACK_MAX_BOXES ? M : 1;       // the buffers a careless caller might bring
      Run r(S >= 1 ? S : 1, Ma);
      memset(r.state.data(), 0x5a, r.state.size());
      const std::vector<unsigned char> before = r.state;
      r.counts[0] = c0;
      const char* why = frmap_track_step_twin(r.state.data(), r.boxes.data(), r.probs.data(), r.counts.data(), r.hw.data(), S, M, 0.9, 0.3,
                                              r.ids.data(), r.rois.data());
      const bool untouched = before == r.state && r.ids[0] == 12345 && r.rois[0] == 12345;
      printf("reject %s %s\n", why ? "refused" : "ACCEPTED", untouched ? "untouched" : "WRITTEN");
    } else {
      fprintf(stderr, "track_twin_check: unknown record %s\n", w.c_str());
      return 2;
    }
  }
  return any ? 0 : self_check();
}
