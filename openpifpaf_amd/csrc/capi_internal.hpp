// What the two files of the C ABI (capi.hip: decoder, CifDet, profiler; capi_trunk.hip: the trunk's producer kernels and
// preprocessing) share.  Defined once in capi.hip; hidden, so the library's dynamic symbol table holds the C ABI and nothing of this.
#pragma once

#include "common.hpp"

#include <string>

namespace opa {

__attribute__((visibility("hidden"))) int fail(int code, const std::string& msg);          // -> code; msg is what opa_last_error answers
__attribute__((visibility("hidden"))) int fail_hip(hipError_t e, const char* where);       // -> OPA_ERR_HIP, "<where>: <HIP's text>"
__attribute__((visibility("hidden"))) size_t align_up(size_t v, size_t a = 256);

}  // namespace opa
