// ldpc_dispatch.hpp -- host side shared by the three launchers of the
// small-code kernels (ldpc_kernels.hip, ldpc_ring.hip, ldpc_serve.hip): the
// one runtime-to-template dispatch, and the per-device / per-kernel figures a
// launch is sized with.  Each launcher keeps what is its own: the launch, its
// largest slot count and its MINB policy.  The launchers of the
// workgroup-per-frame kernels (ldpc_onchip.hip, ldpc_layered.hip) size theirs
// with resident_workgroups / wg_launch at the end of this file.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "ldpc_kernels.hpp"

#ifndef LDPC_TP_MINB
#define LDPC_TP_MINB 4  // throughput build: four waves per SIMD (<= 128 VGPRs)
#endif

#pragma GCC visibility push(hidden)

namespace ldpc {

// kernel_shape (ldpc_kernels.hpp) at degrees that make a cell low / generic:
// .low != low where the rule has no low cell (NW = 4, slots > 4).
constexpr KernelShape cell_shape(int nw, int slots, bool low) {
  return kernel_shape(nw, slots, low ? 0 : kDcMax, low ? 0 : kDvMax);
}

// One instantiation of the small-code kernels, as a type: what dispatch_small
// hands to its functor.  DCN / DVN are the shape rule's, so the kernel's loop
// lengths are the ones the layout was planned for.
template <int PREC_, int METHOD_, int S_, int NW_, bool LOW_>
struct SmallCell {
  static constexpr int PREC = PREC_, METHOD = METHOD_, S = S_, NW = NW_;
  static constexpr bool LOW = LOW_;
  static_assert(cell_shape(NW, S, LOW).low == LOW, "no low-degree cell at this NW and slot count");
  static constexpr int DCN = cell_shape(NW, S, LOW).dcn, DVN = cell_shape(NW, S, LOW).dvn;
};

namespace dispatch {

// slots -> S.  MAXS: the caller's largest slot count; a low cell exists only
// where the shape rule has one (NW = 1, slots <= 4).  Cells past either are
// not instantiated.
template <int MAXS, int PREC, int METHOD, int NW, bool LOW, class F>
int by_slots(int slots, F &f) {
  auto at = [&](auto s) -> int {
    constexpr int S = decltype(s)::value;
    if constexpr (S <= MAXS && cell_shape(NW, S, LOW).low == LOW)
      return f(SmallCell<PREC, METHOD, S, NW, LOW>{});
    else
      return -2;
  };
  switch (slots) {
    case 1: return at(std::integral_constant<int, 1>{});
    case 2: return at(std::integral_constant<int, 2>{});
    case 3: return at(std::integral_constant<int, 3>{});
    case 4: return at(std::integral_constant<int, 4>{});
    case 5: return at(std::integral_constant<int, 5>{});
    case 6: return at(std::integral_constant<int, 6>{});
    case 7: return at(std::integral_constant<int, 7>{});
    case 8: return at(std::integral_constant<int, 8>{});
    default: return -2;
  }
}
static_assert(kSlotsMax == 8, "by_slots lists the slot counts");

template <int MAXS, int PREC, int METHOD, int NW, class F>
int by_shape(const KernelShape &shape, int slots, F &f) {
  return shape.low ? by_slots<MAXS, PREC, METHOD, NW, true>(slots, f)
                   : by_slots<MAXS, PREC, METHOD, NW, false>(slots, f);
}

template <int MAXS, int NW, class F>
int by_method(int method, int prec, const KernelShape &shape, int slots, F &f) {
  if (method == 1) {
    if (prec == 1) return by_shape<MAXS, 1, 1, NW>(shape, slots, f);
    if (prec == 2) return by_shape<MAXS, 2, 1, NW>(shape, slots, f);
    if (prec == 3) return by_shape<MAXS, 3, 1, NW>(shape, slots, f);
    return by_shape<MAXS, 0, 1, NW>(shape, slots, f);
  }
  if (method == 0)  // min-sum has no transcendentals: both f64 modes are the same arithmetic
    return prec == 1 ? by_shape<MAXS, 1, 0, NW>(shape, slots, f)
                     : by_shape<MAXS, 0, 0, NW>(shape, slots, f);
  return -2;
}

}  // namespace dispatch

// Calls f(SmallCell<PREC, METHOD, S, NW, LOW>{}) for the instantiation that
// (method 0 / 1, prec, slots, nw) and the code's shape pick, and returns its
// result; -2 for a shape no kernel is built for (slots > MAXS, nw not 1 or 4,
// another method).  `shape` is kernel_shape(nw, slots, dc_max, dv_max) of the
// code (a caller whose kernel has the generic loops only passes the generic
// shape).
template <int MAXS, class F>
int dispatch_small(int method, int prec, int slots, int nw, const KernelShape &shape, F f) {
  if (nw == 1) return dispatch::by_method<MAXS, 1>(method, prec, shape, slots, f);
  if (nw == 4) return dispatch::by_method<MAXS, 4>(method, prec, shape, slots, f);
  return -2;
}

// CUs of device `dev`, looked up once per device (256 when the query fails).
int cu_count(int dev);

// Resident workgroups per CU of kernel `fn` at `threads` threads and `lds`
// bytes of dynamic LDS, at most `cap`: computed on the first call and kept in
// `once`, one per kernel instantiation (the same on every MI355X of a box;
// racing threads compute the same value).  Raises the kernel's dynamic-LDS
// limit first when lds > 64 KiB.  0: that failed.
int resident_per_cu(std::atomic<int> &once, const void *fn, int threads, size_t lds, int cap);

// Workgroups the current device holds of kernel `fn` at `threads` threads and
// `lds` bytes of dynamic LDS, for the workgroup-per-frame kernels
// (ldpc_onchip.hip, ldpc_layered.hip): computed when `cache` is 0 and kept
// there.  The LDS size is the code's, so the cache is the context's
// (ldpc_ctx::Onchip::resident, Layered::resident, q8_resident), reset with the
// layout -- resident_per_cu's one word per kernel instantiation would hand one
// code's figure to another.  The kernel's dynamic-LDS limit is raised to
// `lds_limit` first: the attribute belongs to the kernel, not to this code, so
// it allows any layout the planner accepts.  False on a runtime error of the
// attribute or the occupancy query; the CU count is cu_count's, 256 where the
// device does not answer (more workgroups than it holds then queue up behind
// each other: none waits on another).
bool resident_workgroups(const void *fn, int threads, int lds, int lds_limit, int &cache);

// The shape of one workgroup-per-frame launch, the host's half of
// wg_next_frame (ldpc_wgframe.hpp): a.waves, the resident workgroups or one per
// frame of a smaller batch, and *advance_out, what the launch adds to its
// queue counter -- one add per frame decoded, each workgroup's last being the
// one past the batch, so a.B; 0 with a fixed stride.  False when
// resident_workgroups fails.
bool wg_launch(const void *fn, int threads, int lds, int &cache, DecodeArgs &a,
               uint32_t *advance_out);

}  // namespace ldpc

#pragma GCC visibility pop
