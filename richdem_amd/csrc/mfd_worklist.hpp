// mfd_worklist.hpp -- the work list that the engines on D-infinity / MFD proportions run on (mfd.hip: accumulation;
// mfd_distance.hip: distance and drop down; mfd_distance_up.hip: distance and rise up; mfd_reverse.hip: reverse
// accumulation): the seed compaction, the two kernels and the host loop.  What an engine does to a cell is its STEP, a functor passed to the kernels by value:
//
//   uint32_t step(uint32_t c, bool from_list)   one step for the finished cell c; returns the neighbours of c that THIS
//                                               thread finished by it, as a mask of neighbour numbers (bit m - 1)
//   int step.width()                            the raster's width (the kernels form nbr_cell(c, m, width))
//
// from_list is true only for a cell read from the launch's list, i.e. finished in an earlier launch (or a seed).  A
// thread continues inline with the lowest neighbour of the mask; where the others go is what the two kernels differ in.
#pragma once

#include "mfd_shared.hpp"

#include <utility>

namespace rdgpu {

// ---- ready flags -> work list (count / scan / fill; flags are cleared) ------------------------------
constexpr int CPB = 4096;
static __global__ __launch_bounds__(NTHR) void k_rdy_count(const uint8_t *__restrict__ f, uint64_t n, uint32_t *counts) {
  __shared__ uint32_t ws[NTHR / 64];
  const uint64_t base = (uint64_t)blockIdx.x * CPB;
  uint32_t cnt = 0;
#pragma unroll 4
  for (int j = 0; j < CPB / NTHR; j++) {
    const uint64_t c = base + (uint64_t)j * NTHR + threadIdx.x;
    if (c < n && f[c]) cnt++;
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
static __global__ __launch_bounds__(1024) void k_rdy_scan(uint32_t *counts, uint32_t m, uint32_t *total) {
  __shared__ uint32_t part[1024];
  const uint32_t chunk = (m + 1023u) / 1024u;
  const uint32_t lo = threadIdx.x * chunk, hi = min(lo + chunk, m);
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; i++) s += counts[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    uint32_t v = (threadIdx.x >= (uint32_t)o) ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t v = counts[i];
    counts[i] = run;
    run += v;
  }
  if (threadIdx.x == 1023) *total = part[1023];
}
static __global__ __launch_bounds__(NTHR) void k_rdy_fill(uint8_t *f, uint64_t n, const uint32_t *__restrict__ offsets,
                                                          uint32_t *__restrict__ out) {
  __shared__ uint32_t ws[NTHR / 64];
  const uint64_t base = (uint64_t)blockIdx.x * CPB;
  uint32_t run = offsets[blockIdx.x];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = 0; j < CPB / NTHR; j++) {
    const uint64_t c = base + (uint64_t)j * NTHR + threadIdx.x;
    const bool hit = c < n && f[c];
    if (hit) f[c] = 0;
    const unsigned long long bal = __ballot(hit);
    const uint32_t rank = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) ws[wv] = __popcll(bal);
    __syncthreads();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NTHR / 64; k++) {
      const uint32_t v = ws[k];
      if (k < wv) woff += v;
      tot += v;
    }
    if (hit) out[run + woff + rank] = (uint32_t)c;
    run += tot;
    __syncthreads();
  }
}

constexpr int WL_BUF = 20;     // entries of a thread's buffer (k_wl_buffer)
constexpr int WL_CAP = 1536;   // entries of a wavefront's stack (k_wl_stack: 4 x 6 KB of LDS per block)
constexpr uint32_t NOCELL = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t nbr_cell(uint32_t c, int m, int w) {
  return (uint32_t)((int)c + mdy(m) * w + mdx(m));
}

// Every thread takes one cell of the launch's list and continues inline with the first neighbour it finishes; the others
// go into the thread's LDS buffer, and at the end the block appends all buffered cells to the next launch's list with ONE
// counter add (same-address atomics serialise at ~12 ns on this chip, and full-raster flag compaction cost 4 ms per
// launch x hundreds of launches: r01b FA_Tarboton 1.2 s at 40k x 40k).  A thread whose buffer could not take a worst
// case (8 neighbours) hands its current cell over to the next launch unprocessed.
template <class STEP>
__global__ __launch_bounds__(NTHR) void k_wl_buffer(STEP step, const uint32_t *__restrict__ list, uint32_t nlist,
                                                    uint32_t *next_list, uint32_t *next_count) {
  __shared__ uint32_t buf[WL_BUF][NTHR];
  __shared__ uint32_t wtot[NTHR / 64];
  __shared__ uint32_t bbase;
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  uint32_t nb = 0;
  if (i < nlist) {
    uint32_t c = list[i];
    for (bool from_list = true;; from_list = false) {
      if (nb + 8 > WL_BUF) { buf[nb++][threadIdx.x] = c; break; }
      uint32_t done = step(c, from_list);
      if (!done) break;
      const uint32_t c0 = c;
      c = nbr_cell(c0, __builtin_ctz(done) + 1, step.width());
      for (done &= done - 1u; done; done &= done - 1u)
        buf[nb++][threadIdx.x] = nbr_cell(c0, __builtin_ctz(done) + 1, step.width());
    }
  }
  // block-wide exclusive prefix of nb, one counter add per block
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t incl = nb;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wtot[wv] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t tot = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    bbase = tot ? atomicAdd(next_count, tot) : 0;
  }
  __syncthreads();
  uint32_t off = bbase + incl - nb;
  for (int k = 0; k < wv; k++) off += wtot[k];
  for (uint32_t k = 0; k < nb; k++) next_list[off + k] = buf[k][threadIdx.x];
}

// The same step with the by-products consumed where they arise (r04f).  In k_wl_buffer a cell finished "on the side" waits
// for the next launch, and a launch lasts as long as its longest inline chain: the accumulation at S3 where every cell
// drains, 2614 launches of 2.8 ms.  Here a wavefront keeps a STACK of such cells in LDS: a lane whose chain has ended takes
// the next cell from it in the same trip of the loop, so a launch ends when everything reachable from its list is done --
// except what a full stack spills to the next launch's list.  All lanes of a wavefront run the loop together (ballots
// decide), the stack pointer is wave-uniform, LDS operations of one wavefront execute in order: no barriers.
template <class STEP>
__global__ __launch_bounds__(NTHR) void k_wl_stack(STEP step, const uint32_t *__restrict__ list, uint32_t nlist,
                                                   uint32_t *next_list, uint32_t *next_count) {
  __shared__ uint32_t stack[NTHR / 64][WL_CAP];
  volatile uint32_t *const sk = stack[threadIdx.x >> 6];
  const int lane = threadIdx.x & 63;
  uint32_t sp = 0;   // (wave-uniform)
  const uint32_t i = blockIdx.x * NTHR + threadIdx.x;
  uint32_t c = i < nlist ? list[i] : NOCELL;
  for (bool from_list = true;; from_list = false) {   // nothing is popped in the first trip: the stack is empty
    const unsigned long long idle = __builtin_amdgcn_ballot_w64(c == NOCELL);
    if (idle == ~0ull && sp == 0) break;
    if (idle != 0ull && sp != 0) {   // idle lanes take the top of the stack
      const uint32_t k = min((uint32_t)__popcll(idle), sp);
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
      if (c == NOCELL && rank < k) c = sk[sp - 1u - rank];
      sp -= k;
    }
    uint32_t oth = 0, c0 = c;
    if (c != NOCELL) {
      const uint32_t done = step(c, from_list);
      c = done ? nbr_cell(c0, __builtin_ctz(done) + 1, step.width()) : NOCELL;   // continue inline with the first one,
      oth = done & (done - 1u);                                                  // the others go on the stack
    }
    const uint32_t no = (uint32_t)__popc(oth);
    if (__builtin_amdgcn_ballot_w64(no != 0u) != 0ull) {   // push the step's by-products: one prefix over the lanes
      uint32_t incl = no;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      uint32_t pos = incl - no;
      if (sp + total <= (uint32_t)WL_CAP) {
        for (; oth; oth &= oth - 1u) sk[sp + pos++] = nbr_cell(c0, __builtin_ctz(oth) + 1, step.width());
        sp += total;
      } else {   // the stack cannot take them: the next launch's list
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(next_count, total);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        for (; oth; oth &= oth - 1u) next_list[base + pos++] = nbr_cell(c0, __builtin_ctz(oth) + 1, step.width());
      }
    }
  }
}

// The seeds (the cells flagged in ready, n of them in all), once, by flag compaction; afterwards every launch appends its
// successor list itself.  Lists of stack_below cells or more go through k_wl_buffer (launch name round_name), shorter ones
// through k_wl_stack (stack_name); the engines say why, where they choose stack_below.  Returns the number of work-list
// launches.  The scratch planes are shared by the engines (never in use at the same time: one call per device at a time).
template <class STEP>
static uint32_t worklist_run(uint8_t *ready, uint64_t n, STEP step, const char *round_name, const char *stack_name,
                             uint32_t stack_below, const char *no_end, hipStream_t s) {
  Workspace &ws = Workspace::get();
  uint32_t *hw = ws.host_words();
  uint32_t *list = ws.buf<uint32_t>("mfd.list", n);
  uint32_t *list2 = ws.buf<uint32_t>("mfd.list2", n);
  const uint32_t nblk = (uint32_t)((n + CPB - 1) / CPB);
  uint32_t *counts = ws.buf<uint32_t>("mfd.counts", (size_t)nblk + 1);
  uint32_t *ctr = counts + nblk;
  RD_LAUNCH("mfd.ready_count", k_rdy_count, dim3(nblk), dim3(NTHR), 0, s, (const uint8_t *)ready, n, counts);
  RD_LAUNCH("mfd.ready_scan", k_rdy_scan, dim3(1), dim3(1024), 0, s, counts, nblk, ctr);
  RD_HIP(hipMemcpyAsync(hw, ctr, 4, hipMemcpyDeviceToHost, s));
  RD_HIP(hipStreamSynchronize(s));
  uint32_t nl = hw[0];
  if (nl) RD_LAUNCH("mfd.ready_fill", k_rdy_fill, dim3(nblk), dim3(NTHR), 0, s, ready, n, (const uint32_t *)counts, list);
  uint32_t launches = 0;
  while (nl) {
    RD_HIP(hipMemsetAsync(ctr, 0, sizeof(uint32_t), s));
    if (nl < stack_below)
      RD_LAUNCH(stack_name, (k_wl_stack<STEP>), dim3((nl + NTHR - 1) / NTHR), dim3(NTHR), 0, s, step, (const uint32_t *)list, nl,
                list2, ctr);
    else
      RD_LAUNCH(round_name, (k_wl_buffer<STEP>), dim3((nl + NTHR - 1) / NTHR), dim3(NTHR), 0, s, step, (const uint32_t *)list, nl,
                list2, ctr);
    RD_HIP(hipMemcpyAsync(hw, ctr, 4, hipMemcpyDeviceToHost, s));
    RD_HIP(hipStreamSynchronize(s));
    nl = hw[0];
    std::swap(list, list2);
    if (++launches > (1u << 26)) throw Error(RDGPU_ERR_HIP, no_end);
  }
  return launches;
}

}  // namespace rdgpu
