// BackendCall.h -- how the facade makes ONE call of a batched entry point of the library (include/vislam_ba.h: handle, count, problem
// pointers, result pointers): with this thread's handle, and on failure the message "<who>: <vba_last_error>" on std::cerr, or
// "<who>: no HIP device (the backend has no CPU path)" when there is no handle.  Optimizer.cpp words its own messages.
#pragma once
#include <cstdint>
#include <iostream>

#include "Optimizer.h"

namespace ORB_SLAM2 {

// n problems.  false: the call failed and the message is written
template <class P, class R>
bool BackendCall(const char* who, int (*fn)(void*, int32_t, P* const*, R* const*), int32_t n, P* const* pp, R* const* pr) {
    void* h = Optimizer::BackendHandle();
    if (h && fn(h, n, pp, pr) == 0) return true;
    std::cerr << who << ": " << (h ? vba_last_error(h) : "no HIP device (the backend has no CPU path)") << std::endl;
    return false;
}

// one problem
template <class P, class R>
bool BackendCall(const char* who, int (*fn)(void*, int32_t, P* const*, R* const*), P& p, R& r) {
    P* pp = &p;
    R* pr = &r;
    return BackendCall(who, fn, 1, &pp, &pr);
}

}  // namespace ORB_SLAM2
