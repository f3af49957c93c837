// color_transfer.h -- what both colour transfers run on a target's neighbours and candidates: S18 (PCCPointSet3::transferColors,
// PCCPointSet.cpp:807-1124, uchar4, attributes.hip) and T4 (transferColors16bitBP :1126-1470, ushort4, post_reconstruct.hip).
// Every mean is fp64 in the reference's order of operations, divisions and roots with one rounding.
#pragma once
#include <hip/hip_runtime.h>

#include "cand_sort.h"
#include "color_transfer_rules.h"  // S18 over the encoder's parameters; what follows is its CTC point and T4's constants

namespace tmc2 {

template <typename C4>
__device__ __forceinline__ C4 roundedColor( const ColorSum& v ) {
  using S = decltype( C4().x );  // uint8_t / uint16_t: the clamp is the type's range
  const auto q = []( double x ) { return S( fmax( 0.0, fmin( round( x ), double( S( ~S( 0 ) ) ) ) ) ); };
  return C4{q( v.c0 ), q( v.c1 ), q( v.c2 ), 0};
}

// A target's candidates (.x squared distance, .y entry number) as the reference leaves them: appended by entry number, then
// std::sort by distance (cand_sort.h).  False: the sort hit its depth limit.
__device__ __forceinline__ bool orderCandidates( uint2* e, int n ) {
  for ( int i = 1; i < n; ++i ) {
    const uint2 v = e[i];
    int         k = i - 1;
    while ( k >= 0 && e[k].y > v.y ) {
      e[k + 1] = e[k];
      --k;
    }
    e[k + 1] = v;
  }
  return CandSort{e}.sort( n );
}

// forward: the eight nearest source points (squared distances ds, nearest first); an identical one ("dist < 0.0001") gives its colour
template <typename C4>
__device__ __forceinline__ C4 forwardColor( const uint32_t id[8], const uint32_t ds[8], const C4* __restrict__ src ) {
  if ( ds[0] == 0 ) return src[id[0]];
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, sw = 0.0;
#pragma unroll
  for ( int i = 0; i < 8; ++i ) {
    const double w = __ddiv_rn( 1.0, double( ds[i] ) + 4.0 );
    const C4     c = src[id[i]];
    c0 += double( c.x ) * w;
    c1 += double( c.y ) * w;
    c2 += double( c.z ) * w;
    sw += w;
  }
  return roundedColor<C4>( ColorSum{__ddiv_rn( c0, sw ), __ddiv_rn( c1, sw ), __ddiv_rn( c2, sw )} );
}

// backward: the n >= 1 ordered candidates, candidate k's colour at src[sourceOf( e[k].y )]; a single one counts unweighted
template <typename C4, typename SourceOf>
__device__ __forceinline__ ColorSum backwardColor( const uint2* e, int n, const C4* __restrict__ src, const SourceOf& sourceOf ) {
  if ( n == 1 ) {
    const C4 c = src[sourceOf( e[0].y )];
    return ColorSum{double( c.x ), double( c.y ), double( c.z )};
  }
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, sw = 0.0;
  for ( int k = 0; k < n; ++k ) {
    const C4     c = src[sourceOf( e[k].y )];
    const double d = double( e[k].x );
    const double w = __ddiv_rn( 1.0, __dsqrt_rn( d ) + 4.0 );
    c0 += double( c.x ) * w;
    c1 += double( c.y ) * w;
    c2 += double( c.z ) * w;
    sw += w;
  }
  return ColorSum{__ddiv_rn( c0, sw ), __ddiv_rn( c1, sw ), __ddiv_rn( c2, sw )};
}

// fixWeight: w = 0  ->  round( 0 * forward + 1 * backward )
template <typename C4>
__device__ __forceinline__ C4 combinedColor( const C4 f, const ColorSum& b ) {
  return roundedColor<C4>( ColorSum{0.0 * double( f.x ) + 1.0 * b.c0, 0.0 * double( f.y ) + 1.0 * b.c1, 0.0 * double( f.z ) + 1.0 * b.c2} );
}

}  // namespace tmc2
