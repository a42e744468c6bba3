// What a vnm_type is, for device code (vnm_common.hpp) and for host-only code that never sees a device compiler
// (vnm_project_type.hpp): one definition, the qualifier empty where the compiler knows none.
#pragma once
#include "../../include/vinum_hip.h"

#ifdef __HIPCC__
#define VNM_HOST_DEVICE __host__ __device__
#else
#define VNM_HOST_DEVICE
#endif

namespace vnm {

VNM_HOST_DEVICE inline int type_width(int t) {
    switch (t) {
        case VNM_I8: case VNM_U8: return 1;
        case VNM_I16: case VNM_U16: return 2;
        case VNM_I32: case VNM_U32: case VNM_F32: return 4;
        default: return 8;
    }
}
VNM_HOST_DEVICE inline bool type_is_float(int t) { return t == VNM_F32 || t == VNM_F64; }
VNM_HOST_DEVICE inline bool type_is_unsigned(int t) { return t >= VNM_U8 && t <= VNM_U64; }

}  // namespace vnm
