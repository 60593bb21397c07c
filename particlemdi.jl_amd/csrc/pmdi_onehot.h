// pmdi_onehot.h -- what the kernels that form a contingency table as a product of one-hot int8 matrices share
// (pmdi_mixing.hip: a chain against its own past; pmdi_partdist.hip: every candidate against every draw; pmdi_agreement.hip: a
// dataset against another or against known classes; pmdi_relabel.hip: a state against the pivot): the fragment types of
// v_mfma_i32_32x32x32_i8, the padding byte, the ordering of one wave's LDS accesses, the exact 64-bit sum over a wave, the
// byte compare that makes the one-hot fragments and the packing of a row of int32 labels into bytes.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef int mx_v4i __attribute__((ext_vector_type(4)));
typedef int mx_v16i __attribute__((ext_vector_type(16)));
typedef unsigned mx_v4u __attribute__((ext_vector_type(4)));

#define MX_PAD 255u     // the byte of a label outside 0..N-1 and of the padding behind a row: no one-hot row ever matches it

// orders the LDS accesses of one wave's lanes among themselves (a wave's LDS operations execute in order; this keeps the
// compiler from moving them across): enough for a buffer only this wave touches
__device__ __forceinline__ void mx_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned long long mx_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// sixteen label bytes against one label: byte j of the result is [byte j of w == label], the fragment of a one-hot int8 matrix.
// rep = the label in all four bytes; one = 0x01010101, or 0 for a label that does not exist (>= N: 255 would match MX_PAD).
// Per dword: x = w ^ rep has a zero byte where the labels agree; (x & 0x7f..) + 0x7f.. carries into bit 7 of every byte whose
// low seven bits are not all zero, never across bytes; | x adds the bytes whose bit 7 is set: bit 7 = [byte != 0].
__device__ __forceinline__ mx_v4i mx_onehot(mx_v4u w, unsigned rep, unsigned one)
{
    mx_v4i f;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned x = w[d] ^ rep;
        const unsigned nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7;
        f[d] = (int)(~nz & one);
    }
    return f;
}

// One wavefront turns row p [n] of int32 labels into bytes o [np] (np = n rounded up to 32; the bytes behind n are MX_PAD); a
// lane packs four consecutive labels into one aligned dword.  A label outside 0..N-1 (a negative one is a large one) goes out
// as MX_PAD; the result, the same in every lane, says whether the row held one.
__device__ __forceinline__ bool mx_label_row(const int *__restrict__ p, long long n, int np, int N, unsigned *__restrict__ o, int lane)
{
    unsigned bad = 0u;
    const int nd = np >> 2;
#pragma unroll 4
    for (int j = lane; j < nd; j += 64) {
        unsigned u[4], w = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {                        // every address is clamped into the row and the guard selects
            const long long i = 4ll * j + b;                 // afterwards: no load sits under a branch
            u[b] = (unsigned)p[i < n ? i : n - 1];
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const bool in_row = 4ll * j + b < n, ok = in_row && u[b] < (unsigned)N;
            bad |= (in_row && !ok) ? 1u : 0u;
            w |= (ok ? u[b] : MX_PAD) << (8 * b);
        }
        o[j] = w;
    }
    bad |= (unsigned)__shfl_xor((int)bad, 32); bad |= (unsigned)__shfl_xor((int)bad, 16); bad |= (unsigned)__shfl_xor((int)bad, 8);
    bad |= (unsigned)__shfl_xor((int)bad, 4); bad |= (unsigned)__shfl_xor((int)bad, 2); bad |= (unsigned)__shfl_xor((int)bad, 1);
    return bad != 0u;
}

}  // namespace
