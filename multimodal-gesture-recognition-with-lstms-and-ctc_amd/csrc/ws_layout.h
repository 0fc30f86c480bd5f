// Workspace layouts (plain host C++17, no HIP types).  A workspace is a sequence of blocks, each padded to 256 bytes, and has ONE layout
// function next to its entry point: (base, dims) -> a struct of named block pointers + bytes.  The mgr_*_ws_bytes query is that
// function with a null base.  The functions fill their struct from a braced list, which C++ evaluates left to right: the blocks in
// member order, then bytes (the carver's running offset).
#pragma once
#include <stddef.h>
#include <stdint.h>

// bump carver: only offsets are computed, and applied when a base is given (null base: null blocks, off is the total).  A const
// base is the workspace of another call that is only read.
struct mgr_ws_carver {
  char* base;
  size_t off;
  explicit mgr_ws_carver(const void* b, size_t start = 0) : base(static_cast<char*>(const_cast<void*>(b))), off(start) {}
  template <class T>
  T* take(size_t n) {   // n elements of T, padded to 256 bytes
    const size_t at = off;
    off += (n * sizeof(T) + 255) / 256 * 256;
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
};

// beam.hip: the trie (parent, label: [B][nodes]) and the (parent, label) hash table of [B] << bits entries, 1 << bits
// the first power of two >= 2 * nodes (and >= 64: the table is whole 256-byte lines as it is)
struct mgr_beam_ws { int bits; int32_t *parent, *label; unsigned long long* table; size_t bytes; };
static inline mgr_beam_ws mgr_beam_ws_layout(void* ws, int B, size_t nodes) {
  int bits = 6;
  while (((size_t)1 << bits) < 2 * nodes) ++bits;
  mgr_ws_carver w(ws);
  return {bits, w.take<int32_t>((size_t)B * nodes), w.take<int32_t>((size_t)B * nodes), w.take<unsigned long long>((size_t)B << bits), w.off};
}

// joint.hip: per stream the fp64 class-major emissions E [B][C][row] and the two sets of `beam` prefix arrays A [B][2][beam][2][row]
// (gn row, gb row), then every candidate's ln psi and ln p per stream: PSI, LP [B][M][beam * G].  row = mgr_joint_row(T): laid out
// for T frames (the kernels use T - skip: they fit) plus the one entry the chains fetch ahead.
constexpr int kJointMaxStreams = 4;   // MGR_JOINT_MAX_STREAMS
constexpr size_t mgr_joint_row(int T) { return ((size_t)T + 1 + 1) / 2 * 2; }   // (constexpr: the kernels call it too)
struct mgr_joint_ws { double *E[kJointMaxStreams], *A[kJointMaxStreams], *PSI, *LP; size_t bytes; };
static inline mgr_joint_ws mgr_joint_ws_layout(void* ws, int B, int M, const int* T, const int* C, int G, int beam) {
  mgr_ws_carver w(ws);
  mgr_joint_ws L = {};
  for (int m = 0; m < M && m < kJointMaxStreams; ++m) {
    L.E[m] = w.take<double>((size_t)B * C[m] * mgr_joint_row(T[m]));
    L.A[m] = w.take<double>((size_t)B * 2 * beam * 2 * mgr_joint_row(T[m]));
  }
  L.PSI = w.take<double>((size_t)B * M * beam * G);
  L.LP = w.take<double>((size_t)B * M * beam * G);
  L.bytes = w.off;
  return L;
}
