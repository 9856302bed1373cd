// The hand-over schedule of attention_bx3_kernel's pipelined loop (attn_bx3.hip, PIPE): which 32-key tile each side touches around
// barrier b of a walk over the n tiles it0 .. it0 + n - 1, and in which of the two K and the two V slots of the LDS ring it lies.
//   * K runs one tile ahead of V: the consumers compute S(it + 1) in the interval in which they finish softmax(it) and P.V(it).
//   * In front of barrier b the producers store K(it0 + b) and V(it0 + b - 1); behind it (interval b) the consumers read just those.
//   * The stores in front of barrier b + 1 fall into interval b: they go to the other slot of each ring.
//   * Both sides take barriers(n) barriers: n + 1, or none for an empty walk (a key slice with no tile behind its first boundary).
// Plain constexpr functions of integers: the kernel's two sides index the ring through them, and the host test
// (tests/test_attn_pipeline_schedule_host.py) compiles this file alone and replays the ring for every (it0, n) it is asked about.
#pragma once

namespace ipdm {
namespace attn_pipe {

constexpr int NONE = -1;      // no tile

constexpr int barriers(int n) { return n > 0 ? n + 1 : 0; }
// ... of which the first has only S behind it and the last only P.V; the ones between, b = 1 .. steady(n), have both
constexpr int steady(int n) { return n > 0 ? n - 1 : 0; }

// producers: the tiles stored in front of barrier b
constexpr int k_stored(int it0, int n, int b) { return b >= 0 && b < n ? it0 + b : NONE; }
constexpr int v_stored(int it0, int n, int b) { return b >= 1 && b <= n ? it0 + b - 1 : NONE; }
// ... and fetched from memory in front of barrier b, for the stores in front of barrier b + 1
constexpr int k_loaded(int it0, int n, int b) { return k_stored(it0, n, b + 1); }
constexpr int v_loaded(int it0, int n, int b) { return v_stored(it0, n, b + 1); }

// consumers: the tiles read behind barrier b -- S of k_read, P.V (and the softmax and split in front of it) of v_read
constexpr int k_read(int it0, int n, int b) { return b >= 0 && b < n ? it0 + b : NONE; }
constexpr int v_read(int it0, int n, int b) { return b >= 1 && b <= n ? it0 + b - 1 : NONE; }

// the slot of a tile, in the K ring and in the V ring alike
constexpr int slot(int tile) { return tile & 1; }

}  // namespace attn_pipe
}  // namespace ipdm
