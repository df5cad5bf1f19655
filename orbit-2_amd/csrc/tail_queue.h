// Tail queue of the one-workgroup-per-CU kernels: the last rounds of a launch are handed out by ticket.
//
// Workgroup b of a launch runs on XCD b & 7, so a static tile walk gives every XCD a fixed eighth of the tiles and the launch lasts
// as long as its slowest XCD.  A planned launch of T tiles keeps the static walk for its first S = T - tail tiles (computed with S
// in place of the grid size: no atomic, the L2 cohorts as they were) and launches 2 * tail further workgroups for the last `tail`
// tiles: each of them draws ONE ticket from the launch's counter (relaxed, agent scope); ticket t < tail is tile S + t, any other
// ticket means "nothing left" and the workgroup returns.  An XCD that reaches the tail first draws more of it (up to twice its
// static share).  Nobody waits, polls or sleeps: a workgroup has a tile or it exits.
//
// Counter: one 32-bit word per launch in flight, zero before the launch.  Every one of the 2 * tail workgroups draws exactly one
// ticket, so ticket 2 * tail - 1 is drawn exactly once and is the launch's last access to the word: its drawer stores 0, and the
// word is zero again when the kernel ends (graph replays and back-to-back launches on one stream reuse it without a memset).
// Launches that may run at the same time (different streams) need different words.  A launch that is ABORTED half-way (a fault, a
// reset) leaves the count of the tickets drawn so far in the word: the caller must zero the workspace before it is used again.
//
// The plan and the ticket -> tile rules are plain functions, built host-only by tests/tail_queue_recorder.hip.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define O2_TQ_HD __host__ __device__ __forceinline__
#else
#define O2_TQ_HD inline
#endif

// ---- static tile walks (b = workgroup, nwg = workgroups of the static part; both bijective for any nwg) ----------------------
// every XCD (b & 7) a contiguous range of ids
O2_TQ_HD int o2_xcd_range_id(int b, int nwg) {
  const int xcd = b & 7, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b >> 3);
}
// round-major: the 256 workgroups of a round take 256 consecutive ids, each XCD 32 consecutive ids of those
O2_TQ_HD int o2_xcd_round_id(int b, int nwg) {
  const int base = b & ~255;
  const int cnt = (nwg - base) < 256 ? (nwg - base) : 256;          // workgroups of this round
  const int x = b & 7, s = (b & 255) >> 3;
  const int q8 = cnt >> 3, r8 = cnt & 7;
  return base + (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + s;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------
struct O2TailPlan {
  int S;       // tiles with static ids: workgroups 0 .. S - 1
  int tail;    // tiles taken by ticket: S .. S + tail - 1; 0 = the launch is static (grid = S = T)
  int grid;    // S + 2 * tail (tail workgroups + as many spare ones)
};
#define O2_TQ_MIN_STATIC_ROUNDS 4      // a launch keeps at least this many static rounds in front of its tail, or stays static

// `tail` tiles of T by ticket; any request that does not leave a valid launch (tail <= 0, tail > T, a grid past 2^31) is static
O2_TQ_HD O2TailPlan o2_tail_plan(long long T, long long tail) {
  O2TailPlan p;
  if (T < 0) T = 0;
  if (T > 0x7fffffffLL) { p.S = 0x7fffffff; p.tail = 0; p.grid = p.S; return p; }     // (never launched: grids are 32-bit)
  if (tail <= 0 || tail > T || T + tail > 0x7fffffffLL) tail = 0;
  p.S = (int)(T - tail);
  p.tail = (int)tail;
  p.grid = (int)(T + tail);
  return p;
}
// the tail a launch of T tiles asks for by itself: `rounds` whole rounds of the chip's `slots` workgroup slots, when at least
// O2_TQ_MIN_STATIC_ROUNDS rounds stay static; 0 (static) otherwise, and on a device that is not 256 CUs on 8 XCDs (slots = 0)
O2_TQ_HD long long o2_tail_auto(long long T, int rounds, int slots) {
  if (rounds <= 0 || slots <= 0) return 0;
  const long long tail = (long long)rounds * slots;
  return T >= tail + (long long)O2_TQ_MIN_STATIC_ROUNDS * slots ? tail : 0;
}
// what the entry points' `tail` argument means: 0 = o2_tail_auto, > 0 = that many tiles (tests: small problems with a queued
// part), < 0 = static
O2_TQ_HD O2TailPlan o2_tail_plan_arg(long long T, int tail_arg, int rounds, int slots) {
  return o2_tail_plan(T, tail_arg > 0 ? (long long)tail_arg : tail_arg == 0 ? o2_tail_auto(T, rounds, slots) : 0);
}

// ---- tickets ---------------------------------------------------------------------------------------------------------------------
// the tile of the workgroup that drew `ticket` (-1: none, the workgroup returns), and whether that workgroup zeroes the counter
O2_TQ_HD int o2_tail_ticket_tile(int S, int tail, unsigned int ticket) { return ticket < (unsigned int)tail ? S + (int)ticket : -1; }
O2_TQ_HD bool o2_tail_ticket_resets(int tail, unsigned int ticket) { return ticket == 2u * (unsigned int)tail - 1u; }

// the problem of a grouped launch that owns tile `id` (G: n problems p[i] with their exclusive tile_end), and its first tile
template <class G> O2_TQ_HD int o2_group_problem(const G& g, int id, int& first) {
  int pi = 0;
  while (pi + 1 < g.n && id >= g.p[pi].tile_end) ++pi;
  first = pi ? g.p[pi - 1].tile_end : 0;
  return pi;
}

// kernel argument of a planned launch
struct O2TailQ {
  unsigned int* ctr;
  int S, tail;
};

#if defined(__HIPCC__) || defined(__CUDACC__)
// The tile of this workgroup: static_id(b, S) for b < S, S + ticket for a ticket holder, -1 for a workgroup that returns.
// *is_tail: the tile came by ticket.  slot: 4 bytes of the workgroup's LDS, free on entry and free again on return (the ticket
// goes through it to the other waves).  Workgroup-uniform; every thread of the workgroup must call it.
template <class F>
__device__ __forceinline__ int o2_tail_tile(const O2TailQ& q, F&& static_id, int* slot, bool* is_tail) {
  const int b = (int)blockIdx.x;
  *is_tail = b >= q.S;
  if (b < q.S) return static_id(b, q.S);
  if (threadIdx.x == 0) {
    const unsigned int t = __hip_atomic_fetch_add(q.ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o2_tail_ticket_resets(q.tail, t)) __hip_atomic_store(q.ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *slot = o2_tail_ticket_tile(q.S, q.tail, t);
  }
  __syncthreads();
  const int id = *slot;
  __syncthreads();
  return id;
}

// Diagnostic build only (-DO2_TQ_TRACE; tools/tail_idle.py, never the shipped library): every workgroup of the one-workgroup-per-CU
// kernels leaves [start, end, XCC id] -- the 100 MHz real-time counter of wave 0 at the kernel's entry and behind a barrier at its
// exit, and the hardware's XCC_ID register (bits 3:0), which says on which XCD workgroup b really ran.
#ifdef O2_TQ_TRACE
#define O2_TQ_TRACE_WGS 65536
#define O2_TQ_TRACE_DEFINE(BUF, READER)                                                                    \
  __device__ unsigned long long BUF[O2_TQ_TRACE_WGS * 3];                                                  \
  extern "C" int READER(unsigned long long* host_dst, int n) {                                             \
    return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(BUF), sizeof(unsigned long long) * (size_t)n);    \
  }
#define O2_TQ_TRACE_BEGIN() const unsigned long long tq_t0__ = __builtin_amdgcn_s_memrealtime()
// BASE: the kernel's first record (the attention backward's two passes run in one call: dQ at 0, dK + dV at half the buffer)
#define O2_TQ_TRACE_END(BUF, BASE)                                                                         \
  do {                                                                                                     \
    __syncthreads();                                                                                       \
    if (threadIdx.x == 0 && blockIdx.x + (BASE) < O2_TQ_TRACE_WGS) {                                       \
      unsigned long long* r__ = BUF + ((size_t)blockIdx.x + (BASE)) * 3;                                   \
      r__[0] = tq_t0__;                                                                                    \
      r__[1] = __builtin_amdgcn_s_memrealtime();                                                           \
      r__[2] = (unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20);                              \
    }                                                                                                      \
  } while (0)
#else
#define O2_TQ_TRACE_DEFINE(BUF, READER)
#define O2_TQ_TRACE_BEGIN()
#define O2_TQ_TRACE_END(BUF, BASE)
#endif

// workgroup slots of the current device when it is the part the tail queue is sized for (256 CUs on 8 XCDs: one workgroup per CU,
// workgroup b on XCD b & 7), 0 otherwise -- a launch then stays static
static inline int o2_tail_slots() {
  static int cached[64];               // per device: 0 unknown, -1 not that part, else the slot count
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (cached[dev] == 0) {
    int cus = 0, xccs = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    if (hipDeviceGetAttribute(&xccs, hipDeviceAttributeNumberOfXccs, dev) != hipSuccess) xccs = 0;
    if (cus == 0 || xccs == 0) (void)hipGetLastError();      // (a refused query must not read as the next launch's error)
    cached[dev] = (cus == 256 && xccs == 8) ? cus : -1;
  }
  return cached[dev] > 0 ? cached[dev] : 0;
}
// the tail plan of a launch of T tiles whose caller offers a counter (sched; nullptr: static) -- tail_arg as in o2_tail_plan_arg,
// rounds: what the kernel family asks for by itself; the device is asked only when the launch sizes its own tail
static inline O2TailPlan o2_tail_plan_launch(long long T, const void* sched, int tail_arg, int rounds) {
  if (!sched || tail_arg < 0) return o2_tail_plan(T, 0);
  return o2_tail_plan_arg(T, tail_arg, rounds, tail_arg == 0 ? o2_tail_slots() : 0);
}
// the counter and `tail` the entry points take: one 4-byte aligned word, which only a static call (tail < 0) may leave out
static inline bool o2_sched_ok(const void* sched_ws, int tail) { return sched_ws ? !((uintptr_t)sched_ws & 3) : tail < 0; }
#endif
