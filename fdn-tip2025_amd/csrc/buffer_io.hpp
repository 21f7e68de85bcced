// Raw-buffer access for every kernel file (included by common.hpp, after its fdn_f32x2 / fdn_u32x2 / fdn_u32x4 typedefs): the one
// resource constructor and the fp32 loads / stores of 1, 2, 4 and 8 values.  Per-lane byte offsets are computed once (invalid lanes
// get OOB, an offset past num_records: such a load gives 0, such a store is dropped - K, N and plane tails for free) and the channel
// plane is a scalar offset, so plane walks cost no vector ALU work.  AUX is the cache-policy word of the instruction (0 = default;
// fdsa_tail.hpp reads its hand-off with sc1).
#pragma once

typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef float fdn_f32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned OOB = 0x80000000u;       // tensors are limited to < 2 GB so that OOB (+ small immediates) stays out of range
__device__ __forceinline__ rsrc_t mk_rsrc(const void* base, unsigned bytes) {               // raw buffer, stride 0
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

template <int AUX = 0>
__device__ __forceinline__ float bload(rsrc_t r, unsigned voff, unsigned soff) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, AUX));
}
template <int AUX = 0>
__device__ __forceinline__ fdn_f32x2 bload2(rsrc_t r, unsigned voff, unsigned soff) {
    const fdn_u32x2 u = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, AUX);
    return fdn_f32x2{__uint_as_float(u.x), __uint_as_float(u.y)};
}
template <int AUX = 0>
__device__ __forceinline__ fdn_f32x4 bload4(rsrc_t r, unsigned voff, unsigned soff) {
    const fdn_u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, AUX);
    return fdn_f32x4{__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)};
}
__device__ __forceinline__ void bstore(float v, rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, voff, soff, 0);
}
__device__ __forceinline__ void bstore2(fdn_f32x2 v, rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b64(fdn_u32x2{__float_as_uint(v.x), __float_as_uint(v.y)}, r, voff, soff, 0);
}
__device__ __forceinline__ void bstore4(fdn_f32x4 v, rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b128(fdn_u32x4{__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)}, r, voff, soff, 0);
}
__device__ __forceinline__ void bstore8(const float (&v)[8], rsrc_t r, unsigned voff, unsigned soff) {
    bstore4(fdn_f32x4{v[0], v[1], v[2], v[3]}, r, voff, soff);
    bstore4(fdn_f32x4{v[4], v[5], v[6], v[7]}, r, voff + 16u, soff);
}

// VEC = 1, 2 or 4 consecutive floats per lane as one vector value (register v of it feeds MFMA chain v)
template <int VEC> struct VecT { typedef float type __attribute__((ext_vector_type(VEC))); };
template <int VEC>
__device__ __forceinline__ typename VecT<VEC>::type bloadv(rsrc_t r, unsigned voff, unsigned soff) {
    static_assert(VEC == 1 || VEC == 2 || VEC == 4, "4-, 8- or 16-byte lanes");
    if constexpr (VEC == 4) return bload4(r, voff, soff);
    else if constexpr (VEC == 2) return bload2(r, voff, soff);
    else return typename VecT<1>::type{bload(r, voff, soff)};
}
template <int VEC>
__device__ __forceinline__ void bstorev(typename VecT<VEC>::type f, rsrc_t r, unsigned voff, unsigned soff) {
    static_assert(VEC == 1 || VEC == 2 || VEC == 4, "4-, 8- or 16-byte lanes");
    if constexpr (VEC == 4) bstore4(f, r, voff, soff);
    else if constexpr (VEC == 2) bstore2(f, r, voff, soff);
    else bstore(f[0], r, voff, soff);
}
