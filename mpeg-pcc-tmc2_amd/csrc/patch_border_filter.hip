// patch_border_filter.hip -- T7, occupancy synthesis (the reference: patch border filtering) on gfx950: what
// PCCCodec::generatePointCloud runs first when pbfEnableFlag_ is set (PccLibCommon/source/PCCCodec.cpp:543-556).
//
// Replaces (reference: source/lib/...)
//   PatchBlockFiltering::patchBorderFiltering   PccLibCommon/source/PCCPatch.cpp:950-976
//   PCCPatch::setLocalData :797-839, generateBorderPoints3D :851-869, filtering :871-948, isBorder :841-850
//
// The reference walks the patches one after the other; the only thing a patch reads of the others are their border points,
// which exist before any patch is filtered.  So every step is pixel-parallel over all patches at once, one workgroup per 16x16
// patch block through the tile list of the reconstruction (d_tilePatch / PlaceDev):
//   (a) local maps      padded occupancy + int16 depth of every patch, back to back in one pool
//   (b) border points   12-neighbour stencil; box per patch by integer atomic min / max (LDS first, one global atomic per
//                       block and bound); the points by a wave-compacted append, each with its (patch, raster index)
//   (c) landings        one lane per border point over the patches whose box meets its own patch's: ONE 64-bit atomicMin per
//                       landing on (distance, source patch, raster index, sign of d - depth) -- the minimum is "the first among
//                       the nearest in the reference's order" (neighbour patches ascending, their points in raster order),
//                       whatever the order of arrival; decoded into the int16 neighbour depths, where the reference's
//                       comparison with the initial 32767 is applied
//   (d) passes          one launch per pass, patch_border_filter.h's pbfKeepPixel per pixel (fp64 roots, float sums)
//   (e) border flags    isBorder of every interior pixel
// The reconstruction (attributes.hip) then reads the filtered map for its occupancy test and the flags for the boundary types.
// No host round trip: the number of border points stays on the device (the landing pass strides over it).
#include <vector>

#include "internal.h"
#include "patch_border_filter.h"
#include "wave.h"

namespace tmc2 {
namespace {

struct PbfPoint {  // a border point: its position, the patch it comes from, its raster index there
  int16_t  p[3];
  uint16_t patch;
  uint32_t raster, pad;
};
constexpr unsigned long long kNoLanding = ~0ull;

// the pixel of this lane: tile -> patch k, pixel (u, v) of the patch, canvas pixel (x, y), ownership of the block
struct TilePixel {
  uint32_t k;
  int      u, v, x, y;
  bool     owned;
};
__device__ __forceinline__ TilePixel tilePixel( const PlaceDev* __restrict__ place, const uint32_t* __restrict__ tilePatch,
                                                const uint32_t* __restrict__ blockToPatch, int W, PlaceDev& p ) {
  TilePixel t;
  t.k             = tilePatch[blockIdx.x];
  p               = place[t.k];
  const int local = int( blockIdx.x ) - p.tileBase;
  const int ub = local % p.sizeU0, vb = local / p.sizeU0;
  const int bx = p.orient == 0 ? ub + p.u0 : vb + p.u0, by = p.orient == 0 ? vb + p.v0 : ub + p.v0;
  t.owned = blockToPatch[size_t( by ) * ( W / 16 ) + bx] == t.k + 1;
  t.u = ub * 16 + int( threadIdx.x & 15 ), t.v = vb * 16 + int( threadIdx.x >> 4 );
  t.x = p.orient == 0 ? t.u + p.u0 * 16 : t.v + p.u0 * 16;
  t.y = p.orient == 0 ? t.v + p.v0 * 16 : t.u + p.v0 * 16;
  return t;
}

// ---- (a) ----------------------------------------------------------------------------------------------------
// (the pools are zero: only occupied pixels are written)
__global__ __launch_bounds__( 256 ) void pbfLocalMapsKernel( const PlaceDev* __restrict__ place, const uint32_t* __restrict__ tilePatch,
                                                              const uint32_t* __restrict__ blockToPatch, const uint8_t* __restrict__ occVideo,
                                                              const uint16_t* __restrict__ geo0, int W, int H, int prec, int b, int thresholdLossyOM,
                                                              const int64_t* __restrict__ offset, uint8_t* __restrict__ occ,
                                                              int16_t* __restrict__ depth ) {
  PlaceDev        p;
  const TilePixel t = tilePixel( place, tilePatch, blockToPatch, W, p );
  if ( !t.owned || t.x >= W || t.y >= H ) return;
  if ( int( occVideo[size_t( t.y / prec ) * ( W / prec ) + t.x / prec] ) <= thresholdLossyOM ) return;
  const int64_t c = offset[t.k] + int64_t( t.v + b ) * ( p.sizeU0 * 16 + 2 * b ) + t.u + b;
  occ[c]          = 1;
  depth[c]        = int16_t( geo0[size_t( t.y ) * W + t.x] );
}

// ---- (b) ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__( 256 ) void pbfBorderPointsKernel( const PlaceDev* __restrict__ place, const uint32_t* __restrict__ tilePatch, int b,
                                                                 const int64_t* __restrict__ offset, const uint8_t* __restrict__ occ,
                                                                 const int16_t* __restrict__ depth, int* __restrict__ box /* [P][6] */,
                                                                 PbfPoint* __restrict__ points, uint32_t* __restrict__ pointCount ) {
  __shared__ int  sbox[6];
  const uint32_t  k     = tilePatch[blockIdx.x];
  const PlaceDev  p     = place[k];
  const int       local = int( blockIdx.x ) - p.tileBase;
  const int       u = ( local % p.sizeU0 ) * 16 + int( threadIdx.x & 15 ), v = ( local / p.sizeU0 ) * 16 + int( threadIdx.x >> 4 );
  const int       w = p.sizeU0 * 16 + 2 * b;
  const int64_t   c = int64_t( v + b ) * w + u + b;
  if ( threadIdx.x < 6 ) sbox[threadIdx.x] = threadIdx.x < 3 ? 32767 : -32768;
  __syncthreads();
  const bool isPoint = pbfIsBorderPoint( occ + offset[k], c, w );
  int16_t    q[3]    = {0, 0, 0};
  if ( isPoint ) {
    q[p.axT] = int16_t( u + p.u1 );
    q[p.axB] = int16_t( v + p.v1 );
    q[p.axN] = int16_t( pbfNormalCoord( p.mode, p.d1, depth[offset[k] + c] ) );
    for ( int a = 0; a < 3; ++a ) {
      atomicMin( &sbox[a], int( q[a] ) );
      atomicMax( &sbox[3 + a], int( q[a] ) );
    }
  }
  // wave-compacted append: one returning add per wave that has points
  const unsigned long long mask = __ballot( isPoint );
  const int                lane = threadIdx.x & 63;
  uint32_t                 base = 0;
  if ( mask != 0ull ) {
    const int leader = __ffsll( (long long)mask ) - 1;
    if ( lane == leader ) base = atomicAdd( pointCount, uint32_t( __popcll( mask ) ) );
    base = __shfl( base, leader, 64 );
  }
  if ( isPoint ) {
    PbfPoint pt;
    pt.p[0] = q[0], pt.p[1] = q[1], pt.p[2] = q[2];
    pt.patch  = uint16_t( k );
    pt.raster = uint32_t( v ) * uint32_t( p.sizeU0 * 16 ) + uint32_t( u );
    pt.pad    = 0;
    points[base + uint32_t( laneRank( mask, lane ) )] = pt;
  }
  __syncthreads();
  if ( threadIdx.x < 3 && sbox[threadIdx.x] != 32767 ) atomicMin( &box[k * 6 + threadIdx.x], sbox[threadIdx.x] );
  if ( threadIdx.x >= 3 && threadIdx.x < 6 && sbox[threadIdx.x] != -32768 ) atomicMax( &box[k * 6 + threadIdx.x], sbox[threadIdx.x] );
}

__device__ __forceinline__ PbfBox loadBox( const int* __restrict__ box, uint32_t k ) {
  PbfBox r;
  for ( int a = 0; a < 3; ++a ) r.lo[a] = int16_t( box[k * 6 + a] ), r.hi[a] = int16_t( box[k * 6 + 3 + a] );
  return r;
}

// ---- (c) ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__( 256 ) void pbfLandingsKernel( const PlaceDev* __restrict__ place, uint32_t P, int b, const int64_t* __restrict__ offset,
                                                             const int16_t* __restrict__ depth, const int* __restrict__ box,
                                                             const PbfPoint* __restrict__ points, const uint32_t* __restrict__ pointCount,
                                                             int reach, unsigned long long* __restrict__ landing ) {
  const uint32_t n = *pointCount;
  for ( uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x ) {
    const PbfPoint pt   = points[i];
    const PbfBox   mine = loadBox( box, pt.patch );
    for ( uint32_t k = 0; k < P; ++k ) {
      if ( k == pt.patch ) continue;
      const PbfBox other = loadBox( box, k );
      if ( !pbfBoxesMeet( other, mine ) || !pbfInGrownBox( other, pt.p ) ) continue;
      const PlaceDev q = place[k];
      const int      w = q.sizeU0 * 16 + 2 * b, h = q.sizeV0 * 16 + 2 * b;
      const int      cu = int( pt.p[q.axT] ) - q.u1 + b, cv = int( pt.p[q.axB] ) - q.v1 + b;
      if ( cu < 0 || cv < 0 || cu >= w || cv >= h ) continue;  // (only a coordinate that wrapped in its int16 gets here)
      const int64_t c    = offset[k] + int64_t( cv ) * w + cu;
      const int     diff = pbfDepthIn( q.mode, q.d1, pt.p[q.axN] ) - int( depth[c] );
      const int     dist = diff < 0 ? -diff : diff;
      if ( dist > reach ) continue;
      const unsigned long long key = ( (unsigned long long)dist << 47 ) | ( (unsigned long long)pt.patch << 31 ) |
                                     ( (unsigned long long)pt.raster << 1 ) | ( diff < 0 ? 1ull : 0ull );
      atomicMin( &landing[c], key );
    }
  }
}

// the nearest landing of every pixel as the reference's int16 neighbour depth; the candidate had to beat the initial 32767
__global__ __launch_bounds__( 256 ) void pbfNeighbourDepthKernel( const unsigned long long* __restrict__ landing, const int16_t* __restrict__ depth,
                                                                   int64_t total, int16_t* __restrict__ nd ) {
  const int64_t i = int64_t( blockIdx.x ) * blockDim.x + threadIdx.x;
  if ( i >= total ) return;
  const unsigned long long key = landing[i];
  int                      v   = kPbfUndefined;
  if ( key != kNoLanding ) {
    const int dist = int( key >> 47 ), own = depth[i];
    const int held = kPbfUndefined - own;  // (never negative)
    if ( dist < held ) v = ( key & 1ull ) ? own - dist : own + dist;
  }
  nd[i] = int16_t( v );
}

// ---- (d) ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__( 256 ) void pbfPassKernel( const PlaceDev* __restrict__ place, const uint32_t* __restrict__ tilePatch, int b,
                                                         const int64_t* __restrict__ offset, const uint8_t* __restrict__ src,
                                                         const int16_t* __restrict__ depth, const int16_t* __restrict__ nd, int filterSize,
                                                         uint8_t* __restrict__ dst ) {
  const uint32_t k     = tilePatch[blockIdx.x];
  const PlaceDev p     = place[k];
  const int      local = int( blockIdx.x ) - p.tileBase;
  const int      u = ( local % p.sizeU0 ) * 16 + int( threadIdx.x & 15 ), v = ( local / p.sizeU0 ) * 16 + int( threadIdx.x >> 4 );
  const int      w = p.sizeU0 * 16 + 2 * b;
  const int64_t  o = offset[k], c = int64_t( v + b ) * w + u + b;
  dst[o + c]       = pbfKeepPixel( src + o, depth + o, nd + o, c, w, filterSize );
}

// ---- (e) ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__( 256 ) void pbfBorderFlagKernel( const PlaceDev* __restrict__ place, const uint32_t* __restrict__ tilePatch, int b,
                                                               const int64_t* __restrict__ offset, const uint8_t* __restrict__ occ,
                                                               uint8_t* __restrict__ flag ) {
  const uint32_t k     = tilePatch[blockIdx.x];
  const PlaceDev p     = place[k];
  const int      local = int( blockIdx.x ) - p.tileBase;
  const int      u = ( local % p.sizeU0 ) * 16 + int( threadIdx.x & 15 ), v = ( local / p.sizeU0 ) * 16 + int( threadIdx.x >> 4 );
  const int      w = p.sizeU0 * 16 + 2 * b;
  const int64_t  o = offset[k], c = int64_t( v + b ) * w + u + b;
  flag[o + c]      = pbfBorderFlag( occ + o, c, w );
}

__global__ __launch_bounds__( 256 ) void pbfInitBoxKernel( int* __restrict__ box, uint32_t P, uint32_t* __restrict__ pointCount ) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i == 0 ) *pointCount = 0;
  if ( i < P * 6 ) box[i] = ( i % 6 ) < 3 ? 32767 : -32768;
}

}  // namespace

// The filter on the frame's canvases.  Leaves f->pbfOcc / f->pbfFlag (padded maps, all patches back to back at f->d_pbfOffset)
// and f->havePbf; everything is queued on the context's stream, nothing is waited for.
int patchBorderFilterDevice( tmc2_frame* f, const PbfParams& q ) {
  if ( !f->haveGeometryImages ) {
    setError( "generatePointCloud (patch border filtering): geometry images missing" );
    return TMC2_E_STATE;
  }
  const uint32_t P = uint32_t( f->patches.size() );
  if ( const char* what = pbfRefusal( f->occPrecision, q, long( P ) ) ) {
    setError( "generatePointCloud (patch border filtering): unsupported %s", what );
    return TMC2_E_UNSUPPORTED;
  }
  tmc2_ctx*   ctx = f->ctx;
  hipStream_t s   = ctx->stream;
  const int   W = f->canvasW, H = f->canvasH, prec = f->occPrecision, b = pbfBorder( prec );
  f->havePbf = false;
  f->pbfOffset.assign( size_t( P ) + 1, 0 );
  for ( uint32_t k = 0; k < P; ++k ) {
    const tmc2_patch& t = f->patches[size_t( f->packOrder[k] )];
    f->pbfOffset[k + 1] = f->pbfOffset[k] + int64_t( t.sizeU0 * 16 + 2 * b ) * int64_t( t.sizeV0 * 16 + 2 * b );
  }
  const int64_t  total = f->pbfOffset[P];
  const uint32_t tiles = f->tileCount;
  if ( total >= ( int64_t( 1 ) << 31 ) * 256 ) {
    setError( "generatePointCloud (patch border filtering): %lld padded pixels unsupported", (long long)total );
    return TMC2_E_UNSUPPORTED;
  }
  DevBuf<int16_t>            d_depth, d_nd;
  DevBuf<unsigned long long> d_landing;
  DevBuf<int>                d_box;
  DevBuf<PbfPoint>           d_points;
  DevBuf<uint32_t>           d_count;
  TMC2_TRY( f->d_pbfOffset.alloc( size_t( P ) + 1 ) );
  TMC2_TRY( f->d_pbfMapA.alloc( size_t( std::max<int64_t>( total, 1 ) ) ) );
  TMC2_TRY( f->d_pbfMapB.alloc( size_t( std::max<int64_t>( total, 1 ) ) ) );
  TMC2_TRY( d_depth.alloc( size_t( std::max<int64_t>( total, 1 ) ) ) );
  TMC2_TRY( d_nd.alloc( size_t( std::max<int64_t>( total, 1 ) ) ) );
  TMC2_TRY( d_landing.alloc( size_t( std::max<int64_t>( total, 1 ) ) ) );
  TMC2_TRY( d_box.alloc( size_t( std::max( P, 1u ) ) * 6 ) );
  TMC2_TRY( d_points.alloc( std::max<size_t>( size_t( tiles ) * 256, 1 ) ) );  // (at most every interior pixel is a border point)
  TMC2_TRY( d_count.alloc( 1 ) );
  StageScope stage( ctx, "patch_border_filter" );
  TMC2_HIP( hipMemcpyAsync( f->d_pbfOffset.p, f->pbfOffset.data(), ( size_t( P ) + 1 ) * sizeof( int64_t ), hipMemcpyHostToDevice, s ) );
  const dim3 blk( 256 );
  hipLaunchKernelGGL( pbfInitBoxKernel, dim3( ( P * 6 + 256 ) / 256 ), blk, 0, s, d_box.p, P, d_count.p );
  if ( total > 0 && tiles > 0 ) {
    TMC2_TRY( fillRegions( ctx, {{f->d_pbfMapA.p, size_t( total ), 0},
                                 {f->d_pbfMapB.p, size_t( total ), 0},
                                 {d_depth.p, size_t( total ) * sizeof( int16_t ), 0},
                                 {d_landing.p, size_t( total ) * sizeof( unsigned long long ), 0xFF}} ) );
    uint8_t *      a = f->d_pbfMapA.p, *other = f->d_pbfMapB.p;
    const int64_t* off = f->d_pbfOffset.p;
    hipLaunchKernelGGL( pbfLocalMapsKernel, dim3( tiles ), blk, 0, s, f->d_place.p, f->d_tilePatch.p, f->d_blockToPatch.p, f->d_occVideo.p,
                        f->d_geo.p, W, H, prec, b, q.thresholdLossyOM, off, a, d_depth.p );
    hipLaunchKernelGGL( pbfBorderPointsKernel, dim3( tiles ), blk, 0, s, f->d_place.p, f->d_tilePatch.p, b, off, a, d_depth.p, d_box.p,
                        d_points.p, d_count.p );
    hipLaunchKernelGGL( pbfLandingsKernel, dim3( cappedBlocks( ctx, tiles ) ), blk, 0, s, f->d_place.p, P, b, off, d_depth.p, d_box.p,
                        d_points.p, d_count.p, q.log2Threshold * q.log2Threshold, d_landing.p );
    hipLaunchKernelGGL( pbfNeighbourDepthKernel, dim3( uint32_t( ( total + 255 ) / 256 ) ), blk, 0, s, d_landing.p, d_depth.p, total, d_nd.p );
    for ( int pass = 0; pass < q.passesCount; ++pass ) {
      hipLaunchKernelGGL( pbfPassKernel, dim3( tiles ), blk, 0, s, f->d_place.p, f->d_tilePatch.p, b, off, a, d_depth.p, d_nd.p, q.filterSize,
                          other );
      std::swap( a, other );
    }
    hipLaunchKernelGGL( pbfBorderFlagKernel, dim3( tiles ), blk, 0, s, f->d_place.p, f->d_tilePatch.p, b, off, a, other );
    f->pbfOcc = a, f->pbfFlag = other;
  } else {
    f->pbfOcc = f->d_pbfMapA.p, f->pbfFlag = f->d_pbfMapB.p;
  }
  TMC2_HIP( hipGetLastError() );
  stage.end();
  // (the temporaries go back to the pool when this returns: the pool hands a block out again only to work queued on the same stream)
  f->pbfBorderWidth = b;
  f->pbfParams[0] = q.thresholdLossyOM, f->pbfParams[1] = q.passesCount, f->pbfParams[2] = q.filterSize, f->pbfParams[3] = q.log2Threshold;
  f->havePbf = true;
  return TMC2_OK;
}

}  // namespace tmc2

extern "C" {

int tmc2_codec_generate_point_cloud_pbf( tmc2_frame* f, int thresholdLossyOM, int passesCount, int filterSize, int log2Threshold ) {
  if ( !f ) return TMC2_E_INVALID;
  tmc2::ApiScope        scope( f->ctx );
  const tmc2::PbfParams q{thresholdLossyOM, passesCount, filterSize, log2Threshold};
  return tmc2::reconstructPointCloud( f, &q );
}

int tmc2_frame_patch_border_filtering_size( tmc2_frame* f, int64_t* pixels ) {
  if ( !f || !pixels ) return TMC2_E_INVALID;
  if ( !f->havePbf ) {
    tmc2::setError( "patch_border_filtering_size: the frame has no filtered maps (tmc2_codec_generate_point_cloud_pbf first)" );
    return TMC2_E_STATE;
  }
  int64_t n = 0;
  for ( size_t k = 0; k < f->patches.size(); ++k ) {
    const tmc2_patch& t = f->patches[size_t( f->packOrder[k] )];
    n += int64_t( t.sizeU0 ) * t.sizeV0 * 256;
  }
  *pixels = n;
  return TMC2_OK;
}

int tmc2_frame_get_patch_border_filtering( tmc2_frame* f, uint8_t* occupancy, uint8_t* border ) {
  if ( !f ) return TMC2_E_INVALID;
  if ( !f->havePbf ) {
    tmc2::setError( "get_patch_border_filtering: the frame has no filtered maps (tmc2_codec_generate_point_cloud_pbf first)" );
    return TMC2_E_STATE;
  }
  tmc2::ApiScope scope( f->ctx );
  hipStream_t    s     = f->ctx->stream;
  const size_t   P     = f->patches.size();
  const size_t   total = size_t( f->pbfOffset[P] );
  const int      b     = f->pbfBorderWidth;
  std::vector<uint8_t> h( std::max<size_t>( total, 1 ) );
  for ( int which = 0; which < 2; ++which ) {
    uint8_t* out = which == 0 ? occupancy : border;
    if ( !out || total == 0 ) continue;
    TMC2_HIP( hipMemcpyAsync( h.data(), which == 0 ? f->pbfOcc : f->pbfFlag, total, hipMemcpyDeviceToHost, s ) );
    TMC2_HIP( hipStreamSynchronize( s ) );
    size_t at = 0;
    for ( size_t k = 0; k < P; ++k ) {
      const tmc2_patch& t = f->patches[size_t( f->packOrder[k] )];
      const int         w = t.sizeU0 * 16 + 2 * b;
      for ( int v = 0; v < t.sizeV0 * 16; ++v, at += size_t( t.sizeU0 ) * 16 )
        std::memcpy( out + at, h.data() + size_t( f->pbfOffset[k] ) + size_t( v + b ) * w + b, size_t( t.sizeU0 ) * 16 );
    }
  }
  return TMC2_OK;
}
}
