// The LDS-DMA weight ring of the streamed MLP kernels (mlp16.hip, nonrigid16.hip, the split-operand kernels of mlp.hip and
// nonrigid.hip, the fused trunk forward of trunks.hip), and the one LDS-DMA statement of csrc/ (linear.hip issues it too,
// into a single-buffered chunk: no ring there).
//
// The scheme.  A workgroup's weights are one stream of equal chunks (kChunkUnits x 16 B) in global memory.  The workgroup
// fetches every chunk ONCE, by LDS-DMA, into slot c & (kSlots - 1) of a ring in LDS, and all its waves read it from there
// with ds_read_b128.  Each wave issues kPieces pieces of 1 KiB (64 lanes x 16 B) per chunk, the same pieces of every
// chunk.  In steady state a wave has three chunks outstanding when it enters one:
//
//     wait_oldest()        s_waitcnt vmcnt(2 * kPieces): the DMAs of one wave retire in order, so all but the two youngest
//                          chunks' pieces -- this wave's share of the chunk being entered -- have landed; two chunks stay
//                          in flight across
//     s_barrier            (raw: __syncthreads() would drain vmcnt) every wave's share has landed: the chunk is whole.
//                          Every wave has also finished with the PREVIOUS chunk -- it waited for its ds_reads of it
//                          before the barrier (wait_oldest_and_lds), or holds it in registers that an MFMA before the
//                          barrier consumed -- so that chunk's slot is free
//     slot(c)              read the chunk
//     piece()/chunk()      refill the freed slot with the chunk kSlots - 1 ahead, wherever the kernel's schedule wants the
//                          pieces (behind which MFMA is the kernel's business: the ring owns addresses, counts and the DMA
//                          statement, no policy)
//
// and drain() before the kernel ends.  The read-ahead runs past the end of the stream, so the packers append zero chunks
// that nobody computes with: kAhead of them, one more (kTailChunks) for a kernel that enters a chunk ahead of the one it
// multiplies.  (A persistent kernel whose stream wraps passes a stream index of its own to piece(): ring position and
// stream position differ after the first wrap.)
//
// What the count rests on.
//   * vmcnt counts EVERY vector-memory instruction of the wave, and loads, stores and DMAs retire out of order with respect
//     to each other: the counted wait means "chunk landed" only while DMAs alone are in flight.  The kernels therefore load
//     their inputs and side data BEFORE the first piece is issued and store their results after the last chunk.  trunks.hip
//     stores activations in mid-stream; its store phases are the exception and say how they restore the invariant.
//   * The compiler does not see the DMA (inline asm) and must not: for a DMA it can see it drains vmcnt(0) before the first
//     ds_read.  For the same reason the kernel keeps ONE __shared__ object, ring first, its other LDS behind -- a second
//     object makes hipcc drain vmcnt before every ds_read.
//   * The source address is a wave-uniform base (SGPR pair) + 32-bit lane offset: a vector-memory instruction whose address
//     is a 64-bit VGPR pair per lane holds up the issuing SIMD's matrix pipe for ~40 cycles on gfx950, whatever it moves.
#pragma once

#include "common.h"

namespace occ {

// LDS-DMA of 64 x 16 B: lane i reads gbase + lane_off(i) and lands at lds_dst + 16 i (M0 carries the wave-uniform LDS
// destination; it is compiler-reserved, so the statement saves and restores it itself).
__device__ __forceinline__ void glds16(const void *gbase, unsigned lane_off, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(lane_off), "s"(gbase), "s"(lds_dst)
                 : "memory");
}

// Stream and ring are counted in 16-byte units, whatever the kernel's operand type (f32x4, eight 2-byte values).
template <int kChunkUnits_, int kPieces_, int kSlots_ = 4>
struct WeightRing {
    static constexpr int kChunkUnits = kChunkUnits_, kPieces = kPieces_, kSlots = kSlots_;
    static constexpr int kAhead = kSlots - 1;           // chunks requested beyond the one entered
    static constexpr int kTailChunks = kSlots;          // zero chunks behind the stream (see above)
    static constexpr int kLdsUnits = kSlots * kChunkUnits;      // the ring's share of the kernel's __shared__ object
    static_assert((kSlots & (kSlots - 1)) == 0, "slot = chunk & (kSlots - 1)");
    static_assert(2 * kPieces < 64, "the wait count is a 6-bit immediate");

    const f32x4 *stream;
    // an LDS pointer, 32 bits: slot addresses formed from the generic pointer cost the trunk forward a VGPR
    const __attribute__((address_space(3))) f32x4 *ring;
    int wave, lane;         // wave: wave-uniform (readfirstlane'd by the caller)

    template <typename T>
    __device__ __forceinline__ WeightRing(const T *stream_, const T *ring_, int wave_, int lane_)
        : stream(reinterpret_cast<const f32x4 *>(stream_)), ring((const __attribute__((address_space(3))) f32x4 *)ring_),
          wave(wave_), lane(lane_) {
        static_assert(sizeof(T) == 16, "the ring counts in 16-byte units");
    }

    // piece f (< kPieces) of this wave's share of stream chunk c_stream -> the slot of ring position c_slot
    __device__ __forceinline__ void piece(int c_slot, int c_stream, int f) const {
        const int frag = wave * kPieces + f;
        glds16(stream + (size_t)c_stream * kChunkUnits + frag * 64, lane * 16,
               (unsigned)(size_t)ring + (unsigned)(((c_slot & (kSlots - 1)) * kChunkUnits + frag * 64) * 16));
    }
    __device__ __forceinline__ void chunk(int c_slot, int c_stream) const {
#pragma unroll
        for (int f = 0; f < kPieces; f++) piece(c_slot, c_stream, f);
    }
    template <typename T>
    __device__ __forceinline__ const T *slot(int c) const {
        return (const T *)(ring + (c & (kSlots - 1)) * kChunkUnits);
    }

    __device__ __forceinline__ static void wait_oldest() {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * kPieces) : "memory");
    }
    // ... and for this wave's ds_reads of the previous chunk (kernels that read a chunk in halves, the second one late)
    __device__ __forceinline__ static void wait_oldest_and_lds() {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * kPieces) : "memory");
    }
    __device__ __forceinline__ static void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

}  // namespace occ
