// rq_dispatch.hpp - run-time bools -> compile-time constants: what every launcher of a kernel template over bools is built on.
// Host code without a HIP dependency: a plain host compiler takes this file alone (tests/dispatch_driver.cpp does).
#pragma once
#include <type_traits>

namespace rq {

// dispatch_bools(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) once: the instantiation of a generic
// lambda for these values, chosen by one run-time switch per bool.  The constants arrive in the order the bools were given.
template <bool... DONE, typename F>
inline void dispatch_bools(F&& f) { f(std::bool_constant<DONE>{}...); }
template <bool... DONE, typename F, typename... REST>
inline void dispatch_bools(F&& f, bool next, REST... rest) {
    if (next) dispatch_bools<DONE..., true>(f, rest...);
    else      dispatch_bools<DONE..., false>(f, rest...);
}

}  // namespace rq
