// What the stand-alone check programs of the head-fitting twins share (head_fit_check.cpp, head_fit_group_check.cpp,
// head_fit_hidden_check.cpp): CHECK, a small deterministic generator and a heap block of exactly its size.  Each program defines
// CHECK_SEED, the start of its own sequence, before it includes this file; its grid and everything it checks stay with it.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "head_fit_twin.h"

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      fprintf(stderr, "FAILED %s: ", #cond);      \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, "\n");                      \
      exit(1);                                    \
    }                                             \
  } while (0)

static uint32_t g_seed = CHECK_SEED;
static uint32_t rnd() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return g_seed >> 8;
}
static float small() { return (float)((int)(rnd() % 129) - 64) / 64.0f; }

template <class T>
struct Block {          // exactly n elements on the heap, every byte `fill`
  T* p;
  size_t n;
  explicit Block(size_t n_, int fill = 0) : p((T*)malloc((n_ ? n_ : 1) * sizeof(T))), n(n_) {
    CHECK(p, "malloc");
    memset(p, fill, (n_ ? n_ : 1) * sizeof(T));
  }
  Block(const Block& o) : p((T*)malloc((o.n ? o.n : 1) * sizeof(T))), n(o.n) { memcpy(p, o.p, o.n * sizeof(T)); }
  Block& operator=(const Block&) = delete;
  ~Block() { free(p); }
  bool same(const Block& o) const { return n == o.n && memcmp(p, o.p, n * sizeof(T)) == 0; }
};
