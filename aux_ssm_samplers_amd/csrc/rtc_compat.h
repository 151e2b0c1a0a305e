// rtc_compat.h -- what the device headers of the sequential cSMC sweep (csmc_sweep.h and what it includes) need when hipRTC compiles them for a
// user-defined Feynman-Kac model (fk_program.hip): hipRTC has no C / C++ library headers (<cmath>, <cstdint>, <cstring> ... do not resolve), provides
// the fixed-width integers only inside __hip_internal, and defines neither INFINITY nor NAN.  Under hipcc this header is empty.
#pragma once
#if defined(__HIPCC_RTC__)
using __hip_internal::int32_t;
using __hip_internal::int64_t;
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
#ifndef INFINITY
#define INFINITY __builtin_huge_valf()
#endif
#ifndef NAN
#define NAN __builtin_nanf("")
#endif
#define AX_MEMCPY __builtin_memcpy
#else
#define AX_MEMCPY memcpy
#endif
