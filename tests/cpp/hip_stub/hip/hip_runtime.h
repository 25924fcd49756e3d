// TEST INFRASTRUCTURE: what the shared host-and-device headers of ergo_uvo_amd/csrc need from <hip/hip_runtime.h> when a stand-alone
// CPU program (tests/cpp/h_fit_host.cpp) includes them under a plain C++ compiler: the function attributes, as nothing.
#pragma once
#define __host__
#define __device__
#define __forceinline__ inline
