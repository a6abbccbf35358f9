// amvs_dispatch.h -- what is compiled in, each list once, and the run-time -> template-argument dispatch over
// such a list.  Plain C++17 (no HIP).  A new patch size, source count, tap count or kNN k is one entry here.
#pragma once
#include <type_traits>
#include <utility>

namespace amvs {

template <int... Vs> using IntList = std::integer_sequence<int, Vs...>;

template <class A, class B> struct Concat;
template <int... As, int... Bs> struct Concat<IntList<As...>, IntList<Bs...>> { using type = IntList<As..., Bs...>; };

using CompiledPatches = IntList<3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29>;   // patch sizes K with kernels of their own
// source views S per reference view, in the two parts the fast sweep step's register-source variants are compiled in:
// amvs_kernels_fast_regs.hip holds the first, built without the packing of f32 pairs (csrc/Makefile), and
// amvs_kernels_fast_regs_packed.hip the second, built as every other unit
using UnpackedRegsSourceCounts = IntList<2, 3, 4, 5>;
using PackedRegsSourceCounts = IntList<6>;
using SourceCounts = Concat<UnpackedRegsSourceCounts, PackedRegsSourceCounts>::type;
using ExtendedTaps = IntList<3, 4, 5, 6, 7>;                                             // extended mode: cost taps per axis
using KnnSizes = IntList<8, 10, 16, 20, 32>;                                             // neighbours k of the kNN statistic

template <int... Vs>
constexpr bool in_list(IntList<Vs...>, int v) { return ((v == Vs) || ...); }

template <int V0, int... Vs>
constexpr int list_max(IntList<V0, Vs...>)
{
    int m = V0;
    ((m = Vs > m ? Vs : m), ...);
    return m;
}

// f(std::integral_constant<int, V>) for the entry V of the list that equals v (inside f, `c()` is that entry as a
// constant expression); `miss` when v is not in the list
template <int... Vs, class R, class F>
R dispatch(IntList<Vs...>, int v, R miss, F &&f)
{
    R r = miss;
    (void)((v == Vs && ((r = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return r;
}

// f(K, S) over the compiled patch sizes and the given source counts; `miss` when either is not in its list
template <class Sources, class R, class F>
R dispatch_ks_of(Sources, int K, int S, R miss, F &&f)
{
    return dispatch(CompiledPatches{}, K, miss, [&](auto k) {
        return dispatch(Sources{}, S, miss, [&](auto s) { return f(k, s); });
    });
}

// ... over all source counts
template <class R, class F>
R dispatch_ks(int K, int S, R miss, F &&f)
{
    return dispatch_ks_of(SourceCounts{}, K, S, miss, std::forward<F>(f));
}

}  // namespace amvs
