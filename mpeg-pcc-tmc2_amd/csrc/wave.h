// wave.h -- the cross-lane idioms of the kernels, written once: inclusive scan, butterfly reduction, rank in a ballot, bitonic sort
// of a wave-private LDS array, exclusive scan over a workgroup.  Device-only.  Each body is the plain shuffle loop (width 64, the
// offsets in the order given), so an fp64 sum adds in one fixed order: every lane ends with the same bits.
//
// Precondition of every function here: all 64 lanes of the wavefront reach the call, converged.  No caller sits under a
// lane-dependent branch, and a loop around a call has a wave-uniform trip count.  (WIDTH < 64: the same of every aligned group of
// WIDTH lanes that calls.  blockExclusive: every wavefront of the workgroup, it holds a barrier.  laneRank is plain arithmetic on a
// ballot the caller took while converged, and may be called by the lanes that need it.)
#pragma once
#include "internal.h"

#if defined( __HIPCC__ )
namespace tmc2 {

// Inclusive prefix sum over the lanes (WIDTH < 64: over every aligned group of WIDTH lanes); lane = threadIdx.x & 63.
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T waveInclusive( T v, int lane ) {
#pragma unroll
  for ( int off = 1; off < WIDTH; off <<= 1 ) {
    const T t = __shfl_up( v, off, 64 );
    if ( ( lane & ( WIDTH - 1 ) ) >= off ) v += t;
  }
  return v;
}

// Butterfly reduction: every lane of an aligned group of WIDTH lanes ends with op over the group.
template <int WIDTH = 64, typename T, typename Op>
__device__ __forceinline__ T waveReduce( T v, Op op ) {
#pragma unroll
  for ( int off = WIDTH / 2; off > 0; off >>= 1 ) v = op( v, T( __shfl_xor( v, off, 64 ) ) );
  return v;
}
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T waveSum( T v ) { return waveReduce<WIDTH>( v, []( T a, T b ) { return a + b; } ); }
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T waveMin( T v ) { return waveReduce<WIDTH>( v, []( T a, T b ) { return min( a, b ); } ); }
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T waveMax( T v ) { return waveReduce<WIDTH>( v, []( T a, T b ) { return max( a, b ); } ); }

// The number of set bits of a ballot below this lane: the lane's place in a stream compaction.
__device__ __forceinline__ int laneRank( unsigned long long ballot, int lane ) { return __popcll( ballot & ( ( 1ull << lane ) - 1ull ) ); }

// Sorts keys[0 .. P) ascending; P a power of two, at least 64 (0: nothing to sort), keys in LDS and private to this wavefront.
// A wavefront-scope fence after every pass orders the LDS traffic of the lanes; the caller fences after its last store to keys.
__device__ __forceinline__ void ldsBitonicSort( uint32_t* keys, int P, int lane ) {
  for ( int k = 2; k <= P; k <<= 1 )
    for ( int j = k >> 1; j > 0; j >>= 1 ) {
      for ( int i = lane; i < P; i += 64 ) {
        const int partner = i ^ j;
        if ( partner > i ) {
          const uint32_t a = keys[i], b = keys[partner];
          if ( ( a > b ) == ( ( i & k ) == 0 ) ) keys[i] = b, keys[partner] = a;
        }
      }
      __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" );
    }
}

// Exclusive prefix sum of one value per thread over a workgroup of WAVES wavefronts, in thread order.  waveTot: LDS [WAVES], holds
// the wavefronts' totals afterwards; one barrier inside, none after it (the caller keeps waveTot untouched until every wavefront has
// read it).  total: the sum over the workgroup.
template <int WAVES>
__device__ __forceinline__ uint32_t blockExclusive( uint32_t v, uint32_t* waveTot ) {
  const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc  = waveInclusive( v, lane );
  if ( lane == 63 ) waveTot[wave] = inc;
  __syncthreads();
  uint32_t before = inc - v;
  for ( int w = 0; w < wave; ++w ) before += waveTot[w];
  return before;
}
template <int WAVES>
__device__ __forceinline__ uint32_t blockExclusive( uint32_t v, uint32_t* waveTot, uint32_t& total ) {
  const uint32_t before = blockExclusive<WAVES>( v, waveTot );
  total                 = 0;
#pragma unroll
  for ( int w = 0; w < WAVES; ++w ) total += waveTot[w];
  return before;
}

}  // namespace tmc2
#endif
