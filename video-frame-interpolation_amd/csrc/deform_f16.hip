#include "deform_pack3.inl"
#include "deform_gather3.inl"
#define DEFORM_ROUTE3_TS half_t
#include "deform_route3.inl"
int launch_deform_f16(const DeformParams &p, hipStream_t s) { return launch_deform16<half_t>(p, s); }
int launch_deform_gather_f16(const DeformParams &p, hipStream_t s) { return launch_deform_gather3<half_t>(p, s); }
int launch_deform_routed_f16(const DeformParams &p, hipStream_t s) { return launch_deform_route3(p, s); }
