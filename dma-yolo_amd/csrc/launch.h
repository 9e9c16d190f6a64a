// Host-side launch glue of every kernel file: the dispatch on storage type, runtime bools and compile-time integers,
// the launch itself, the 16-byte vector contract and the grids of the streaming kernels.  Host code only.
#pragma once
#include "common.h"
#include <initializer_list>
#include <tuple>
#include <type_traits>

template <typename T> struct DType { using type = T; };

// f(DType<float>{}) for dtype 0, f(DType<bf16>{}) for dtype 1, `refuse` for anything else.  f is a generic lambda
// whose body is written once, opening with `using T = typename decltype(tag)::type;`, and returns the entry's int.
template <typename F> inline int by_dtype(int dtype, int refuse, F&& f) {
  if (dtype == 0) return f(DType<float>{});
  if (dtype == 1) return f(DType<bf16>{});
  return refuse;
}
// an int as a lambda argument (read as decltype(n)::value), never as a kernel's template argument
template <int N> using Int = std::integral_constant<int, N>;
// by_dtype for a kernel with a scalar twin: f(tag, nv) with decltype(nv)::value = the elements per 16-byte vector
// when `vec` holds, else 1
template <typename F> inline int by_dtype_vec(int dtype, bool vec, int refuse, F&& f) {
  return by_dtype(dtype, refuse, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return vec ? f(tag, Int<Traits<T>::VW>{}) : f(tag, Int<1>{});
  });
}
// by_flags(b0[, b1[, b2]], f): f(std::bool_constant<b0>{}, ...), the runtime bools turned into tags whose ::value picks
// a kernel's bool template arguments.  f is a generic lambda that holds the one launch and returns the entry's int.
template <size_t I = 0, typename Tup, typename... Tag> inline int by_flags_(const Tup& a, Tag... tags) {
  if constexpr (I + 1 == std::tuple_size_v<Tup>) return std::get<I>(a)(tags...);
  else if (std::get<I>(a)) return by_flags_<I + 1>(a, tags..., std::true_type{});
  else return by_flags_<I + 1>(a, tags..., std::false_type{});
}
template <typename... A> inline int by_flags(A&&... a) { return by_flags_(std::forward_as_tuple(a...)); }
// by_int<3, 5, 7>(v, refuse, f): f(Int<V>{}) for the listed V equal to v, `refuse` for any other v.
// by_int<3, 5, 7>(v, Int<0>{}, f): the same, with f(Int<0>{}) for any other v: a ladder's `default:` instantiation.
// f is a generic lambda that returns the entry's int; it is instantiated for the named values only.
template <int... V, typename F, typename G> inline int by_int_(int v, F&& f, G&& other) {
  int r = 0;
  return ((v == V && (r = f(Int<V>{}), true)) || ...) ? r : other();
}
template <int... V, typename F> inline int by_int(int v, int refuse, F&& f) {
  return by_int_<V...>(v, f, [&] { return refuse; });
}
template <int... V, int D, typename F> inline int by_int(int v, Int<D> other, F&& f) {
  return by_int_<V...>(v, f, [&] { return f(other); });
}

// k<<<grid, block, lds, stream>>>(args...) and the launch status.  Each argument is converted to the kernel's own
// parameter type, so an entry passes its void pointers as they are: the kernel's signature, not a cast at the call,
// types them.  The short form is the streaming kernels' 256 threads and no dynamic LDS.  An entry with several
// launches chains them, `if (int e = launch(...)) return e;`: a failed launch returns at once and the later ones are
// not enqueued.  (static: an instantiation the compiler does not inline stays out of the library's exports.)
template <typename... P, typename... A>
static inline int launch(void (*k)(P...), dim3 grid, dim3 block, size_t lds, void* stream, A... args) {
  k<<<grid, block, lds, (hipStream_t)stream>>>(static_cast<P>(args)...);
  return (int)hipGetLastError();
}
template <typename... P, typename... A> static inline int launch(void (*k)(P...), dim3 grid, void* stream, A... args) {
  return launch(k, grid, 256, 0, stream, args...);
}

inline int vec_width(int dtype) { return dtype ? 8 : 4; }  // elements per 16-byte vector
inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }  // a null pointer passes

// The 16-byte vector contract of a streaming kernel: the channel count and every pixel stride are whole vectors of VW
// elements, the `req` bases are non-null and 16-byte aligned, the `opt` bases are aligned when given.  What only one
// kernel needs (a row fitting its stride, a cap on the vectors per row, the SM layout's 4 K) stays at its call site.
inline bool vec_ok(int VW, int C, std::initializer_list<long> strides, std::initializer_list<const void*> req,
                   std::initializer_list<const void*> opt = {}) {
  if (C % VW) return false;
  for (long s : strides)
    if (s % VW) return false;
  for (const void* p : req)
    if (!p || !al16(p)) return false;
  for (const void* p : opt)
    if (!al16(p)) return false;
  return true;
}
// every pixel stride holds a whole row of C channels
inline bool rows_fit(int C, std::initializer_list<long> strides) {
  for (long s : strides)
    if (s < C) return false;
  return true;
}

// grid of the grid-stride elementwise kernels: blocks of 256 threads, capped at 16384 (DMA-1536 step 157.61 / 157.98
// -> 158.13 / 158.32 img/s against 8192, alternating on one box, profiles/r05/elt_grid_ab.log)
constexpr int kEwCap = 16384;
constexpr int kRedCap = 2048;  // blocks (= partial rows) of the row-walking reduce passes, see bn.hip
constexpr int kInvalid = (int)hipErrorInvalidValue;
inline int vgrid(long n) { return grid_cap(ceil_div(n, 256), kEwCap); }
// partial rows of a pass that gives each block 256 pixels: one per block, at least 1, at most cap
inline int part_rows(long M, int cap) { return grid_cap((M + 255) / 256, cap); }
// grid of the row-walking passes (256 threads = RB rows x C / VW channel vectors, 8 loop steps per block)
inline int row_grid(long M, int C, int VW, int cap) { return grid_cap(ceil_div(M, (long)(256 / (C / VW)) * 8), cap); }
// grid of the channel-tile kernels (tile.h): `rows` blocks along x, the tiles of 1 << tcl channel units along y
inline dim3 tile_grid(int rows, int units, int tcl, int z = 1) { return dim3(rows, ceil_div(units, 1 << tcl), z); }
