// voxelize.hip -- the grid-based segmentation (the reference's fast mode, gridBasedSegmentation_) on gfx950.
//
// Replaces PCCPatchSegmenter3::convertPointsToVoxels and applyVoxelsDataToPoints (PccLibEncoder/source/PCCPatchSegmenter.cpp:152-215)
// as the two steps of VoxelCloud, the owner of a frame's voxel cloud.  What PCCPatchSegmenter3::compute runs between them (:78-139)
// is segmenterCompute's (segmenter_api.cpp: the one chain of the segmenter's modes).
//
// The voxel list is in first-occurrence order (voxelize.h).  The first point of every voxel comes out of the stable LSD radix
// sort the metric's de-duplication uses (radix_sort.hip): in a stable sort of (key, point index) pairs the head of a run of equal
// keys is the run's smallest index.  No table is sized by the cube.  Sorted order: run heads, their prefix sum (the run of every
// sorted position), the first point of every run.  Input order: "I am the first of my voxel", its prefix sum (the voxel's rank in
// the list; the total is the voxel count -- the one host round trip, through the context's mailbox), then one pass that stores
// every point's rank and, for the first points, the voxel itself: an order-preserving compaction.
#include <memory>

#include "internal.h"
#include "voxelize.h"

namespace tmc2 {
namespace {

__global__ __launch_bounds__( 256 ) void voxelKeysKernel( const Pt* __restrict__ pts, uint32_t n, VoxelRule r, int axisBits,
                                                           uint64_t* __restrict__ key, uint32_t* __restrict__ index ) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i >= n ) return;
  const Pt p = pts[i];
  key[i]     = voxelKey( voxelCoord( p.x, r ), voxelCoord( p.y, r ), voxelCoord( p.z, r ), axisBits );
  index[i]   = i;
}
// sorted order -> input order: runFirst[run] = the run's first (smallest) point, isFirst[point] = the point is the first of its voxel
// (headsBefore: the exclusive prefix sum of head -- at a head, the number of its run)
__global__ __launch_bounds__( 256 ) void voxelRunFirstKernel( const uint32_t* __restrict__ head, const uint32_t* __restrict__ headsBefore,
                                                               const uint32_t* __restrict__ index, uint32_t n,
                                                               uint32_t* __restrict__ runFirst, uint32_t* __restrict__ isFirst ) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if ( j >= n ) return;
  const uint32_t i = index[j], h = head[j];
  isFirst[i] = h;
  if ( h ) runFirst[headsBefore[j]] = i;
}
// every point takes the rank of its voxel's first point; the first points emit their voxel at that rank
__global__ __launch_bounds__( 256 ) void voxelEmitKernel( const Pt* __restrict__ pts, uint32_t n, VoxelRule r, const uint32_t* __restrict__ head,
                                                           const uint32_t* __restrict__ headsBefore, const uint32_t* __restrict__ index,
                                                           const uint32_t* __restrict__ runFirst, const uint32_t* __restrict__ rank,
                                                           uint32_t voxels, Pt* __restrict__ voxelPts, uint32_t* __restrict__ voxelOfPoint ) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if ( j >= n ) return;
  const uint32_t i = index[j], h = head[j];
  const uint32_t v = rank[runFirst[headsBefore[j] - ( h ? 0u : 1u )]];  // (position 0 is a head: no run "-1")
  voxelOfPoint[i]  = v;
  if ( h && v < voxels ) {
    const Pt p  = pts[i];
    voxelPts[v] = Pt{int16_t( voxelCoord( p.x, r ) ), int16_t( voxelCoord( p.y, r ) ), int16_t( voxelCoord( p.z, r ) ), 0};
  }
}
// applyVoxelsDataToPoints: partition and normal (fp64, bit for bit) of every point = its voxel's
__global__ __launch_bounds__( 256 ) void applyVoxelsKernel( const uint32_t* __restrict__ voxelOfPoint, uint32_t n,
                                                             const uint8_t* __restrict__ partitionVox, const double* __restrict__ normalVox,
                                                             uint8_t* __restrict__ partition, double* __restrict__ normal ) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i >= n ) return;
  const uint32_t v = voxelOfPoint[i];
  partition[i]     = partitionVox[v];
  const size_t a = 3 * size_t( i ), b = 3 * size_t( v );
  normal[a] = normalVox[b], normal[a + 1] = normalVox[b + 1], normal[a + 2] = normalVox[b + 2];
}

}  // namespace

int voxelizeDevice( tmc2_ctx* ctx, const Pt* d_pts, uint32_t n, int voxDim, int maxCoord, DevBuf<Pt>& d_voxelPts, DevBuf<uint32_t>& d_voxelOfPoint,
                    uint32_t* voxelCount ) {
  VoxelRule r;
  if ( !voxelRuleFor( voxDim, r ) || n == 0 || maxCoord < 0 ) {
    setError( "voxelize: invalid argument" );
    return TMC2_E_INVALID;
  }
  hipStream_t      s        = ctx->stream;
  const int        axisBits = voxelAxisBits( voxelCoord( maxCoord, r ) );
  DevBuf<uint64_t> d_keyA, d_keyB;
  DevBuf<uint32_t> d_idxA, d_idxB, d_head, d_headsBefore;
  TMC2_TRY( d_keyA.alloc( n ) );
  TMC2_TRY( d_keyB.alloc( n ) );
  TMC2_TRY( d_idxA.alloc( n ) );
  TMC2_TRY( d_idxB.alloc( n ) );
  TMC2_TRY( d_head.alloc( n ) );
  TMC2_TRY( d_headsBefore.alloc( n ) );
  TMC2_TRY( d_voxelOfPoint.alloc( n ) );
  const dim3 blk( 256 ), grd( ( n + 255 ) / 256 );
  hipLaunchKernelGGL( voxelKeysKernel, grd, blk, 0, s, d_pts, n, r, axisBits, d_keyA.p, d_idxA.p );
  bool inA = true;
  TMC2_TRY( radixSortPairs( ctx, d_keyA.p, d_idxA.p, d_keyB.p, d_idxB.p, n, uint32_t( 3 * axisBits ), &inA ) );
  const uint64_t* key   = inA ? d_keyA.p : d_keyB.p;
  const uint32_t* index = inA ? d_idxA.p : d_idxB.p;
  // the pair of buffers the sort did not end in is free: the runs' first points, and (two words per key) the input-order flags and ranks
  uint32_t* runFirst = inA ? d_idxB.p : d_idxA.p;
  uint32_t* isFirst  = reinterpret_cast<uint32_t*>( inA ? d_keyB.p : d_keyA.p );
  uint32_t* rank     = isFirst + n;
  TMC2_TRY( markRunHeads( ctx, key, n, d_head.p ) );  // head[j] = position j starts a run of equal keys
  TMC2_TRY( exclusiveScanU32( ctx, d_head.p, d_headsBefore.p, n, nullptr ) );
  hipLaunchKernelGGL( voxelRunFirstKernel, grd, blk, 0, s, d_head.p, d_headsBefore.p, index, n, runFirst, isFirst );
  volatile uint32_t* answer = ctx->answerLine( tmc2_ctx::kAnswerVoxelCount );  // (the voxel count straight to a page-locked word: no copy)
  TMC2_TRY( exclusiveScanU32( ctx, isFirst, rank, n, nullptr, ScanAnswer{answer, nullptr, 0} ) );
  TMC2_HIP( hipGetLastError() );
  TMC2_HIP( hipStreamSynchronize( s ) );
  const uint32_t V = answer[0];
  if ( V == 0 || V > n ) {
    setError( "voxelize: %u voxels of %u points", V, n );
    return TMC2_E_HIP;
  }
  TMC2_TRY( d_voxelPts.alloc( V ) );
  hipLaunchKernelGGL( voxelEmitKernel, grd, blk, 0, s, d_pts, n, r, d_head.p, d_headsBefore.p, index, runFirst, rank, V, d_voxelPts.p,
                      d_voxelOfPoint.p );
  TMC2_HIP( hipGetLastError() );
  *voxelCount = V;
  return TMC2_OK;  // (the temporaries go back to the pool; what is queued on the stream runs before their next user's work)
}

int VoxelCloud::build( const tmc2_frame* f, const char* entry, int voxDim, int refineNeighbours ) {
  tmc2_ctx*   ctx = f->ctx;
  hipStream_t s   = ctx->stream;
  frame.reset( new tmc2_frame() );
  frame->ticket.bind( ctx );
  frame->ctx = ctx;
  {
    StageScope span( ctx, "voxelize" );
    TMC2_TRY( voxelizeDevice( ctx, f->d_pts.p, uint32_t( f->n ), voxDim, f->geoMax, frame->d_pts, d_voxelOfPoint, &count ) );
  }
  const uint32_t V = count;
  if ( refineNeighbours == 0 && V < kMinVoxelCloud ) {
    setError( "%s: voxelDimensionGridBasedSegmentation %d leaves a voxel cloud of %u points, fewer than the %u neighbours the normal "
              "estimation asks for",
              entry, voxDim, V, kMinVoxelCloud );
    return TMC2_E_UNSUPPORTED;
  }
  if ( refineNeighbours != 0 && ( V < kMinVoxelCloud || V < uint32_t( refineNeighbours ) ) ) {
    setError( "%s: voxelDimensionGridBasedSegmentation %d leaves a voxel cloud of %u points, fewer than maxNNCountRefineSegmentation %d "
              "or the %u neighbours the normal estimation asks for",
              entry, voxDim, V, refineNeighbours, kMinVoxelCloud );
    return TMC2_E_UNSUPPORTED;
  }
  frame->n = V;
  // the host-resident steps (S3's walk and its point-level fallback, a tree build of option KDTREE_HOST) read h_xyz: once down
  Pt* hp = ctx->hostD.get<Pt>( V );
  if ( !hp ) {
    setError( "%s: hipHostMalloc failed", entry );
    return TMC2_E_HIP;
  }
  TMC2_HIP( hipMemcpyAsync( hp, frame->d_pts.p, size_t( V ) * sizeof( Pt ), hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipStreamSynchronize( s ) );
  frame->h_xyz.resize( 3 * size_t( V ) );
  for ( uint32_t v = 0; v < V; ++v ) {
    frame->h_xyz[3 * size_t( v )] = hp[v].x, frame->h_xyz[3 * size_t( v ) + 1] = hp[v].y, frame->h_xyz[3 * size_t( v ) + 2] = hp[v].z;
    frame->geoMax = std::max( frame->geoMax, std::max( hp[v].x, std::max( hp[v].y, hp[v].z ) ) );
  }
  return TMC2_OK;
}

int VoxelCloud::applyToPoints( tmc2_frame* f, const char* entry ) const {
  if ( !frame->haveNormals || !frame->havePartition ) {
    setError( "%s: the voxel cloud has no normals / partition", entry );
    return TMC2_E_STATE;
  }
  tmc2_ctx*      ctx = f->ctx;
  const uint32_t n   = uint32_t( f->n );
  TMC2_TRY( f->d_normals.alloc( 3 * size_t( n ) ) );
  TMC2_TRY( f->d_partition.alloc( n ) );
  {
    StageScope span( ctx, "voxels_to_points" );
    hipLaunchKernelGGL( applyVoxelsKernel, dim3( ( n + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, d_voxelOfPoint.p, n, frame->d_partition.p,
                        frame->d_normals.p, f->d_partition.p, f->d_normals.p );
    TMC2_HIP( hipGetLastError() );
  }
  f->haveNormals = f->havePartition = true;
  return TMC2_OK;
}

}  // namespace tmc2

using namespace tmc2;

extern "C" {

int tmc2_segmenter_convert_points_to_voxels( tmc2_ctx* ctx, const int16_t* xyz, uint64_t n, int voxDim, int bits, int16_t* voxelXyz,
                                             uint64_t* voxelCount, uint32_t* voxelOfPoint ) {
  if ( !ctx || !xyz || !voxelXyz || !voxelCount || !voxelOfPoint || n == 0 || n > 0x7FFFFFF0ull ) {
    setError( "segmenter_convert_points_to_voxels: invalid argument" );
    return TMC2_E_INVALID;
  }
  TMC2_TRY( voxelizeCheck( "segmenter_convert_points_to_voxels", xyz, n, voxDim, bits ) );
  ApiScope        scope( ctx );
  hipStream_t     s = ctx->stream;
  std::vector<Pt> pts( n );
  int             maxCoord = 0;
  for ( uint64_t i = 0; i < n; ++i ) {
    pts[i] = Pt{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0};
    maxCoord = std::max<int>( maxCoord, std::max( xyz[3 * i], std::max( xyz[3 * i + 1], xyz[3 * i + 2] ) ) );
  }
  DevBuf<Pt>       d_pts, d_voxelPts;
  DevBuf<uint32_t> d_voxelOfPoint;
  TMC2_TRY( d_pts.alloc( n ) );
  TMC2_HIP( hipMemcpyAsync( d_pts.p, pts.data(), n * sizeof( Pt ), hipMemcpyHostToDevice, s ) );
  uint32_t V = 0;
  TMC2_TRY( voxelizeDevice( ctx, d_pts.p, uint32_t( n ), voxDim, maxCoord, d_voxelPts, d_voxelOfPoint, &V ) );
  std::vector<Pt> vp( V );
  TMC2_HIP( hipMemcpyAsync( vp.data(), d_voxelPts.p, size_t( V ) * sizeof( Pt ), hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipMemcpyAsync( voxelOfPoint, d_voxelOfPoint.p, n * sizeof( uint32_t ), hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipStreamSynchronize( s ) );
  for ( uint32_t v = 0; v < V; ++v ) voxelXyz[3 * size_t( v )] = vp[v].x, voxelXyz[3 * size_t( v ) + 1] = vp[v].y, voxelXyz[3 * size_t( v ) + 2] = vp[v].z;
  *voxelCount = V;
  return TMC2_OK;
}

}  // extern "C"
