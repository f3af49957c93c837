// loads.h -- the load batch of the kernels, written once.  Device-only.  What a lane fetches together -- loads none of which is an
// address of another -- is loaded into registers AHEAD of the branches that consume it and pinned there with an empty asm statement
// per value.  Left alone, the compiler sinks every load into the exec-masked block of its first use, behind that block's own
// s_waitcnt vmcnt(0), and takes a 16-byte load apart into the words that are used: a chain of dependent round trips where the source
// reads like a batch.  The statement consumes its value in VGPRs behind the loads (a vector as one tuple): nothing sinks or splits.
//   * pin( a, b, ... ) is ONE asm per value, with no load between them: the waits the compiler puts before them collapse into the
//     first, a batch is one wait.  A value that was not loaded (its predicate failed) is pinned as the constant it was given.
//   * The other form is several operands in one statement: consumed together.  refine.hip's closureHop and sweepKernel keep it for
//     their multi-value batches -- the one-per-value form schedules those two differently.
//   * The rule: a batch keeps the predicate of the serial form on anything that becomes an address.  An index a batch reads early is
//     one the serial form read too, or one valid by construction (i < n, an entry of a k-NN row, a clamped position).
#pragma once
#include "internal.h"

#if defined( __HIPCC__ )
namespace tmc2 {

typedef uint32_t Words2 __attribute__( ( ext_vector_type( 2 ) ) );  // one 8-byte load
typedef uint32_t Words4 __attribute__( ( ext_vector_type( 4 ) ) );  // one 16-byte load
__device__ __forceinline__ void pin( uint32_t& a ) { asm volatile( "" : "+v"( a ) ); }
__device__ __forceinline__ void pin( int32_t& a ) { asm volatile( "" : "+v"( a ) ); }
__device__ __forceinline__ void pin( Words2& a ) { asm volatile( "" : "+v"( a ) ); }
__device__ __forceinline__ void pin( Words4& a ) { asm volatile( "" : "+v"( a ) ); }
template <typename T, typename... Rest>
__device__ __forceinline__ void pin( T& a, Rest&... rest ) {
  pin( a );
  pin( rest... );
}
template <int N>
__device__ __forceinline__ void pinAll( uint32_t ( &a )[N] ) {
#pragma unroll
  for ( int k = 0; k < N; ++k ) pin( a[k] );
}
__device__ __forceinline__ int coordOf( const Pt p, int axis ) { return axis == 0 ? p.x : ( axis == 1 ? p.y : p.z ); }
// a point as its two words (x | y << 16, z | w << 16): one 8-byte load that stays one, decoded from registers
__device__ __forceinline__ Words2 loadPt( const Pt* __restrict__ pts, uint32_t i ) { return reinterpret_cast<const Words2*>( pts )[i]; }
__device__ __forceinline__ Pt ptOf( const Words2 w ) {
  return Pt{int16_t( w.x & 0xFFFFu ), int16_t( w.x >> 16 ), int16_t( w.y & 0xFFFFu ), int16_t( w.y >> 16 )};
}
__device__ __forceinline__ int32_t ptCoord( Words2 p, int axis ) {
  return axis == 0 ? int32_t( int16_t( p.x & 0xFFFFu ) ) : ( axis == 1 ? int32_t( int16_t( p.x >> 16 ) ) : int32_t( int16_t( p.y & 0xFFFFu ) ) );
}
// a whole 16-entry k-NN row in four 16-byte loads (not yet waited for: pin r[0..3] with the rest of the batch)
__device__ __forceinline__ void loadRow16( const uint32_t* __restrict__ knn, uint32_t u, Words4 ( &r )[4] ) {
  const Words4* row = reinterpret_cast<const Words4*>( knn + size_t( u ) * 16 );
#pragma unroll
  for ( int t = 0; t < 4; ++t ) r[t] = row[t];
}
__device__ __forceinline__ void rowEntries( const Words4 ( &r )[4], uint32_t ( &v )[16] ) {
#pragma unroll
  for ( int t = 0; t < 4; ++t ) v[4 * t] = r[t].x, v[4 * t + 1] = r[t].y, v[4 * t + 2] = r[t].z, v[4 * t + 3] = r[t].w;
}

}  // namespace tmc2
#endif
