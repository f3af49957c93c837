// kd_walk.h -- one step of nanoflann's searchLevel (dependencies/nanoflann/nanoflann.hpp:1207-1254) and its computeInitialDistances
// (:901-915) over KdNode records, written once, for the host and the device: where one wrong sign or `<` changes a tie and the lists
// stop being the reference's.  Used by knnKernel, easyQueryKernel (knn.hip), knnWideKernel (knn_wide.hip) and the host search
// (knn_host.h); node load, loop bounds, leaf scan, far-child stack and result list differ for real and stay with them.
// The one restatement: knnSmallTreeKernel (knn.hip) writes the step out over arrays indexed by the node's axis.  Built on kdStep the
// compiler no longer keeps its index list in registers: private memory 1184 -> 1296 bytes and one wait more per insertion, against
// the rule that no kernel's code object gets worse (profiles/kernel_idioms.txt, section 2).  It takes the box from here.
// Every per-axis distance on the way down is the SQUARE of an integer offset (to the root box or to a split plane), so the walk carries
// three offsets.  Squares are summed as uint32_t: the int sum's bits, no overflow for coordinates >= -4096 (3 x 36863^2 < 2^32).
#pragma once
#include <stdlib.h>
#include "cell_grid.h"  // TMC2_HD
#include "internal.h"

namespace tmc2 {

struct KdBox {
  int lo[3], hi[3];
};
inline KdBox kdBoxOf( const int32_t ( &lo )[3], const int32_t ( &hi )[3] ) { return KdBox{{lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}}; }
struct KdOffsets {
  int o0, o1, o2;
};
TMC2_HD int kdAxis( int v0, int v1, int v2, int dim ) { return dim == 0 ? v0 : ( dim == 1 ? v1 : v2 ); }

// computeInitialDistances: the offset of the query to the root box, per axis (0 inside)
TMC2_HD KdOffsets kdInitialOffsets( const KdBox& root, int qx, int qy, int qz ) {
  KdOffsets o = {0, 0, 0};
  if ( qx < root.lo[0] ) o.o0 = root.lo[0] - qx;
  if ( qx > root.hi[0] ) o.o0 = qx - root.hi[0];
  if ( qy < root.lo[1] ) o.o1 = root.lo[1] - qy;
  if ( qy > root.hi[1] ) o.o1 = qy - root.hi[1];
  if ( qz < root.lo[2] ) o.o2 = root.lo[2] - qz;
  if ( qz > root.hi[2] ) o.o2 = qz - root.hi[2];
  return o;
}
// the side test on diff1 = v - divlow, diff2 = v - divhigh (the gap between the children's boxes): left is near; a tie goes right
TMC2_HD bool kdLeftNear( int diff1, int diff2 ) { return diff1 + diff2 < 0; }
// the child on the query's side, the step of the stack-less descent: for ( nd = load( 0 ); nd.dim >= 0; ) nd = load( kdNearChild( .. ) )
TMC2_HD uint32_t kdNearChild( const KdNode& nd, int qx, int qy, int qz ) {
  const int v = kdAxis( qx, qy, qz, nd.dim );
  return kdLeftNear( v - nd.divlow, v - nd.divhigh ) ? uint32_t( nd.a ) : uint32_t( nd.b );
}
// the step at an inner node: near child (offsets as they are), far child (on the node's axis: the distance to its side of the gap)
struct KdStep {
  uint32_t  nearC, farC;
  KdOffsets far;
  uint32_t  farMin;
};
TMC2_HD KdStep kdStep( const KdNode& nd, int qx, int qy, int qz, const KdOffsets o ) {
  const int  v = kdAxis( qx, qy, qz, nd.dim ), ocur = kdAxis( o.o0, o.o1, o.o2, nd.dim );
  const int  diff1 = v - nd.divlow, diff2 = v - nd.divhigh;
  const bool leftNear = kdLeftNear( diff1, diff2 );
  const int  ofar     = leftNear ? abs( diff2 ) : abs( diff1 );
  KdStep     s;
  s.nearC  = leftNear ? uint32_t( nd.a ) : uint32_t( nd.b );
  s.farC   = leftNear ? uint32_t( nd.b ) : uint32_t( nd.a );
  s.far    = KdOffsets{nd.dim == 0 ? ofar : o.o0, nd.dim == 1 ? ofar : o.o1, nd.dim == 2 ? ofar : o.o2};
  s.farMin = uint32_t( o.o0 * o.o0 ) + uint32_t( o.o1 * o.o1 ) + uint32_t( o.o2 * o.o2 ) + uint32_t( ofar * ofar ) - uint32_t( ocur * ocur );
  return s;
}

}  // namespace tmc2
