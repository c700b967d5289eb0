// jb_launch.h -- the one dispatch by output format of the launchers behind the pixel kernel (jb_resample.hip,
// jb_orient.hip, jb_fit.hip, jb_color.hip).  Host code only.
#pragma once
#include <type_traits>

// f(std::integral_constant<int, N>{}) for N = format, a JB_FMT_* in 0..3 (the launcher has checked the range): inside f,
// decltype(F)::value is the kernel's FORMAT template argument
template <class F>
static inline void jb_by_format(int format, F &&f) {
  switch (format) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
  }
}
