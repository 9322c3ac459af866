// plan_table.hpp -- plan tables (host, HIP-free).  A plan family is one
// constexpr table of {a, b} template arguments; for_entry calls a generic
// lambda with the matching entry's two values as std::integral_constants and
// says whether there was one, so the lambda is instantiated for the table's
// entries and nothing else (the product library holds plan-reachable kernels
// only), and every use of a family -- plan, grid, workspace, launch -- names
// its instances through the same table.  Tables: window.hpp (the window
// kernels' bands), reduce_plan.hpp (the row reduce's forms) and the
// translation units' own.
#pragma once

#include <cstddef>
#include <type_traits>
#include <utility>

namespace fedavg_impl {

struct PlanEntry {
  int a, b;
};
constexpr int kAnyB = -1;

template <auto& T, class F, size_t... I>
bool for_entry_impl(int a, int b, F&& f, std::index_sequence<I...>) {
  return ((a == T[I].a && (b == kAnyB || b == T[I].b) &&
           (f(std::integral_constant<int, T[I].a>{}, std::integral_constant<int, T[I].b>{}), true)) ||
          ...);
}
template <auto& T, class F>
bool for_entry(int a, int b, F&& f) {
  return for_entry_impl<T>(a, b, f, std::make_index_sequence<std::extent_v<std::remove_reference_t<decltype(T)>>>{});
}

}  // namespace fedavg_impl
