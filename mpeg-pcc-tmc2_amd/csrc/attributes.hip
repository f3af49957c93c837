// attributes.hip -- phase B on gfx950: point-cloud reconstruction (S17), colour transfer (S18), attribute scatter
// (S20), push-pull background fill (S21) and attribute group dilation (S22).
//
// Replaces (reference: source/lib/...)
//   PCCCodec::generatePointCloud, lossy CTC branch      PccLibCommon/source/PCCCodec.cpp:519-980 (+ generatePoints :329-517,
//                                                       PCCPatch::generatePoint PccLibCommon/include/PCCPatch.h:177-207)
//   PCCPointSet3::transferColors (CTC settings)         PccLibCommon/source/PCCPointSet.cpp:807-1124
//   PCCEncoder::presmoothPointCloudColor                PccLibEncoder/source/PCCEncoder.cpp:6593-6655 -- a no-op in the reference
//                                                       build (boundary type 2 is never produced), therefore skipped
//   PCCEncoder::generateAttributeVideo (per tile)       PCCEncoder.cpp:6736-6794
//   PCCEncoder::dilateSmoothedPushPull / pushPullMip / pushPullFill / mean4w   PCCEncoder.cpp:6357-6591
//   attribute group dilation, inline in PCCEncoder::encode                      PCCEncoder.cpp:380-402
//
// S17 is a stream compaction whose ORDER is part of the contract (patch list order, block raster, pixel raster, D0
// before D1): one workgroup per 16x16 patch block counts its points (ballot + popcount), a prefix sum over the tile
// list gives each tile its output offset, and a second pass emits with an in-tile prefix (wave scan).
// S18 reuses the exact nanoflann-order k-NN kernel: 8-NN of every reconstructed point in the SOURCE tree (the frame's
// own tree) and 1-NN of every source point in a tree built over the reconstruction; the backward votes are bucketed
// per target (count, scan, fill), ordered as the reference's std::sort leaves them and reduced in fp64 in that order: the
// device functions of color_transfer.h, which T4 (post_reconstruct.hip) runs on 16-bit colours.
// S21: every pyramid level is an image-parallel kernel over all six planes (2 maps x RGB) at once.
#include <algorithm>
#include <cmath>

#include "color_transfer.h"
#include "internal.h"
#include "loads.h"
#include "wave.h"
#include "patch_border_filter.h"

namespace tmc2 {
namespace {

__device__ __forceinline__ void toCanvasB( const PlaceDev& p, int u, int v, int& x, int& y ) {
  if ( p.orient == 0 ) {
    x = u + p.u0 * 16;
    y = v + p.v0 * 16;
  } else {
    x = v + p.u0 * 16;
    y = u + p.v0 * 16;
  }
}

__device__ __forceinline__ int normalCoord( const PlaceDev& p, int depth ) {
  return p.mode == 0 ? depth + p.d1 : max( 0, p.d1 - depth );
}

// what the reconstruction reads instead of the occupancy video on a frame with occupancy synthesis (patch_border_filter.hip): the
// filtered per-patch maps and their border flags, padded by `border`, patch k at offset[k]; btype: boundary type per point, out
struct PbfMapsDev {
  const int64_t* offset;
  const uint8_t *occ, *flag;
  int            border;
  uint8_t*       btype;
};

// EMIT = false: tileCount[tile] = number of points of the tile.  EMIT = true: write them at tileOffset[tile].
// PBF: the occupancy test reads the filtered map of the patch, and both points of a pixel take its border flag as boundary type
template <bool EMIT, bool PBF = false>
__global__ __launch_bounds__( 256 ) void reconTileKernel( const PlaceDev* __restrict__ place,
                                                           const uint32_t* __restrict__ tilePatch,
                                                           const uint8_t* __restrict__ occVideo,
                                                           const uint32_t* __restrict__ blockToPatch,
                                                           const uint16_t* __restrict__ geo, int W, int H, int prec,
                                                           uint32_t* __restrict__ tileCount,
                                                           const uint32_t* __restrict__ tileOffset, Pt* __restrict__ recon,
                                                           uint32_t* __restrict__ pointToPixel, PbfMapsDev pbf = PbfMapsDev() ) {
  __shared__ uint32_t waveTotal[4];
  const uint32_t      tile  = blockIdx.x;
  const uint32_t      k     = tilePatch[tile];
  const PlaceDev      p     = place[k];
  const int           local = int( tile ) - p.tileBase;
  const int           ub = local % p.sizeU0, vb = local / p.sizeU0;
  const int           bx = p.orient == 0 ? ub + p.u0 : vb + p.u0, by = p.orient == 0 ? vb + p.v0 : ub + p.v0;
  const bool          owned = blockToPatch[size_t( by ) * ( W / 16 ) + bx] == k + 1;
  const int           u = ub * 16 + int( threadIdx.x & 15 ), v = vb * 16 + int( threadIdx.x >> 4 );
  int                 x, y;
  toCanvasB( p, u, v, x, y );
  uint32_t cnt = 0;
  int      c0 = 0, c1 = 0;
  bool    occupied = owned && x < W && y < H;
  uint8_t flag     = 0;
  if constexpr ( PBF ) {
    if ( occupied ) {
      const int64_t c = pbf.offset[k] + int64_t( v + pbf.border ) * ( p.sizeU0 * 16 + 2 * pbf.border ) + u + pbf.border;
      occupied        = pbf.occ[c] != 0;
      flag            = pbf.flag[c];
    }
  } else {
    occupied = occupied && occVideo[size_t( y / prec ) * ( W / prec ) + x / prec];
  }
  if ( occupied ) {
    c0  = normalCoord( p, geo[size_t( y ) * W + x] );
    c1  = normalCoord( p, geo[size_t( W ) * H + size_t( y ) * W + x] );
    cnt = c1 != c0 ? 2u : 1u;
  }
  // inclusive scan of cnt over the 256 lanes (pixel raster order == lane order)
  const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc  = waveInclusive( cnt, lane );
  if ( lane == 63 ) waveTotal[wave] = inc;
  __syncthreads();
  if ( !EMIT ) {
    if ( threadIdx.x == 0 ) tileCount[tile] = waveTotal[0] + waveTotal[1] + waveTotal[2] + waveTotal[3];
    return;
  }
  if ( cnt == 0 ) return;
  uint32_t off = tileOffset[tile] + inc - cnt;
  for ( int w = 0; w < wave; ++w ) off += waveTotal[w];
  int c[3];
  c[p.axT] = u + p.u1;
  c[p.axB] = v + p.v1;
  c[p.axN] = c0;
  recon[off]        = Pt{int16_t( c[0] ), int16_t( c[1] ), int16_t( c[2] ), 0};
  pointToPixel[off] = packPixel( x, y, 0, cnt == 2 );
  if constexpr ( PBF ) {
    pbf.btype[off] = flag;
    if ( cnt == 2 ) pbf.btype[off + 1] = flag;
  }
  if ( cnt == 2 ) {
    c[p.axN]              = c1;
    recon[off + 1]        = Pt{int16_t( c[0] ), int16_t( c[1] ), int16_t( c[2] ), 0};
    pointToPixel[off + 1] = packPixel( x, y, 1, false );
  }
}

// ---- S18 ------------------------------------------------------------------------------------------------
// easy: the first result of the queries that have an identical source point (0xFFFFFFFF for the others: only
// their rows of idx8 / dist8 are filled -- launchKnnSplit)
__global__ __launch_bounds__( 256 ) void forwardColorKernel( const uint32_t* __restrict__ idx8, const uint32_t* __restrict__ dist8,
                                                              const uint32_t* __restrict__ easy,
                                                              const uint8_t* __restrict__ srcRgb4, uint32_t m,
                                                              uint8_t* __restrict__ fwdRgb4 ) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if ( t >= m ) return;
  if ( easy[t] != 0xFFFFFFFFu ) {  // "dist < 0.0001": an identical source point exists, take its colour
    reinterpret_cast<uchar4*>( fwdRgb4 )[t] = reinterpret_cast<const uchar4*>( srcRgb4 )[easy[t]];
    return;
  }
  const uint4* ir = reinterpret_cast<const uint4*>( idx8 + size_t( t ) * 8 );
  const uint4* dr = reinterpret_cast<const uint4*>( dist8 + size_t( t ) * 8 );
  const uint4  i0 = ir[0], i1 = ir[1], d0 = dr[0], d1 = dr[1];
  const uint32_t id[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
  const uint32_t ds[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
  reinterpret_cast<uchar4*>( fwdRgb4 )[t] = forwardColor( id, ds, reinterpret_cast<const uchar4*>( srcRgb4 ) );
}

// source point s votes for its nearest reconstructed point.  FILL = false: count per target; FILL = true (count: a zeroed cursor):
// place (dist, s) in the target's bucket
template <bool FILL>
__global__ __launch_bounds__( 256 ) void backwardVoteKernel( const uint32_t* __restrict__ idx1, const uint32_t* __restrict__ dist1, uint32_t n,
                                                              uint32_t* __restrict__ count, const uint32_t* __restrict__ offset,
                                                              uint2* __restrict__ entries ) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if ( s >= n ) return;
  const uint32_t t = idx1[s], slot = atomicAdd( &count[t], 1u );
  if ( FILL ) entries[offset[t] + slot] = make_uint2( dist1[s], s );
}

__global__ __launch_bounds__( 256 ) void combineColorKernel( const uint32_t* __restrict__ count, const uint32_t* __restrict__ offset,
                                                              uint2* __restrict__ entries, const uint8_t* __restrict__ srcRgb4,
                                                              const uint8_t* __restrict__ fwdRgb4, uint32_t m,
                                                              uint8_t* __restrict__ outRgb4, uint32_t* __restrict__ error ) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if ( t >= m ) return;
  const int n = int( count[t] );
  if ( n == 0 ) {
    reinterpret_cast<uchar4*>( outRgb4 )[t] = reinterpret_cast<const uchar4*>( fwdRgb4 )[t];
    return;
  }
  uint2* e = entries + offset[t];
  if ( !orderCandidates( e, n ) ) *error = 1;
  // an identical source point comes first and counts alone, unweighted, like a single candidate
  const ColorSum c = backwardColor( e, e[0].x == 0 ? 1 : n, reinterpret_cast<const uchar4*>( srcRgb4 ), []( uint32_t source ) { return source; } );
  reinterpret_cast<uchar4*>( outRgb4 )[t] = combinedColor( reinterpret_cast<const uchar4*>( fwdRgb4 )[t], c );
}

// ---- S18 off the CTC point: the rules of color_transfer_rules.h over rows of `stride` results of which the first k count -----
__device__ __forceinline__ CtColor ctColorOf( const uint8_t* __restrict__ rgb4, uint32_t i ) {
  const uchar4 c = reinterpret_cast<const uchar4*>( rgb4 )[i];
  return CtColor{c.x, c.y, c.z};
}
__device__ __forceinline__ void ctStore( uint8_t* __restrict__ rgb4, uint32_t i, const CtColor& c ) {
  reinterpret_cast<uchar4*>( rgb4 )[i] = make_uchar4( uint8_t( c.c0 ), uint8_t( c.c1 ), uint8_t( c.c2 ), 0 );
}
// easy: nullptr, or launchKnnSplit's first results (only with skipAvgIfIdenticalSourcePointPresentFwd: the rows of those are not filled)
__global__ __launch_bounds__( 256 ) void forwardColorRulesKernel( const uint32_t* __restrict__ idx, const uint32_t* __restrict__ dist, int stride,
                                                                   const uint32_t* __restrict__ easy, const uint8_t* __restrict__ srcRgb4,
                                                                   uint32_t m, CtRules p, uint8_t* __restrict__ fwdRgb4 ) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if ( t >= m ) return;
  if ( easy && easy[t] != 0xFFFFFFFFu ) {
    reinterpret_cast<uchar4*>( fwdRgb4 )[t] = reinterpret_cast<const uchar4*>( srcRgb4 )[easy[t]];
    return;
  }
  const uint32_t* id = idx + size_t( t ) * stride;
  const uint32_t* ds = dist + size_t( t ) * stride;
  ctStore( fwdRgb4, t, ctForward( p, p.kFwd, [ds]( int i ) { return ds[i]; }, [id, srcRgb4]( int i ) { return ctColorOf( srcRgb4, id[i] ); } ) );
}

// source point s votes for each of its kBwd results within the geometry threshold.  FILL = false: count per target; FILL = true
// (count: a zeroed cursor): place (dist, s * kBwd + rank) -- the number of the entry in the order the reference appends them
template <bool FILL>
__global__ __launch_bounds__( 256 ) void backwardVoteRulesKernel( const uint32_t* __restrict__ idx, const uint32_t* __restrict__ dist, int stride,
                                                                   uint32_t n, int kBwd, double geoBwd, uint32_t* __restrict__ count,
                                                                   const uint32_t* __restrict__ offset, uint2* __restrict__ entries ) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if ( s >= n ) return;
  for ( int r = 0; r < kBwd; ++r ) {
    const uint32_t d = dist[size_t( s ) * stride + r];
    if ( !( double( d ) <= geoBwd ) ) continue;
    const uint32_t t = idx[size_t( s ) * stride + r], slot = atomicAdd( &count[t], 1u );
    if ( FILL ) entries[offset[t] + slot] = make_uint2( d, s * uint32_t( kBwd ) + uint32_t( r ) );
  }
}

// One thread per target: the sort replays std::sort's moves one after the other, the shrink loop ends at the first prefix that
// fails, and the best-colour search reads six sums of the list, not the list (color_transfer_rules.h) -- nothing here that the
// lanes of a wavefront could share for one target, long list or not.
__global__ __launch_bounds__( 256 ) void combineColorRulesKernel( const uint32_t* __restrict__ count, const uint32_t* __restrict__ offset,
                                                                   uint2* __restrict__ entries, const uint8_t* __restrict__ srcRgb4,
                                                                   const uint8_t* __restrict__ fwdRgb4, uint32_t m, CtRules p, double rTarget,
                                                                   double rSource, uint8_t* __restrict__ outRgb4, uint32_t* __restrict__ error ) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if ( t >= m ) return;
  const int     n   = int( count[t] );
  const CtColor fwd = ctColorOf( fwdRgb4, t );
  if ( n == 0 || p.lossless ) {
    ctStore( outRgb4, t, fwd );
    return;
  }
  uint2* e = entries + offset[t];
  if ( !orderCandidates( e, n ) ) *error = 1;
  const uint32_t kBwd = uint32_t( p.kBwd );
  ctStore( outRgb4, t,
           ctBackward( p, n, [e]( int i ) { return e[i].x; }, [e, srcRgb4, kBwd]( int i ) { return ctColorOf( srcRgb4, e[i].y / kBwd ); }, fwd,
                       rTarget, rSource ) );
}

// ---- S20 ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__( 256 ) void attributeScatterKernel( const uint8_t* __restrict__ rgb4,
                                                                  const uint32_t* __restrict__ pointToPixel, uint32_t m,
                                                                  int W, int H, uint8_t* __restrict__ attr ) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i >= m ) return;
  const uint32_t pp = pointToPixel[i];
  const size_t   px = size_t( pixelY( pp ) ) * W + pixelX( pp ), plane = size_t( W ) * H;
  const uchar4   c  = reinterpret_cast<const uchar4*>( rgb4 )[i];
  const bool     layer1 = pixelLayer( pp ), hasD1 = pixelHasD1( pp );
  if ( !layer1 ) {
    attr[px] = c.x, attr[plane + px] = c.y, attr[2 * plane + px] = c.z;
    if ( !hasD1 ) attr[3 * plane + px] = c.x, attr[4 * plane + px] = c.y, attr[5 * plane + px] = c.z;
  } else {
    attr[3 * plane + px] = c.x, attr[4 * plane + px] = c.y, attr[5 * plane + px] = c.z;
  }
}

__global__ __launch_bounds__( 256 ) void upsampleOccupancyKernel( const uint8_t* __restrict__ occVideo, int W, int H, int prec,
                                                                   uint8_t* __restrict__ occ ) {
  const size_t c = size_t( blockIdx.x ) * blockDim.x + threadIdx.x;
  if ( c >= size_t( W ) * H ) return;
  occ[c] = occVideo[size_t( ( c / W ) / prec ) * ( W / prec ) + ( c % W ) / prec];
}

// ---- S21 ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mean4w( int p1, int w1, int p2, int w2, int p3, int w3, int p4, int w4 ) {
  return ( p1 * w1 + p2 * w2 + p3 * w3 + p4 * w4 ) / ( w1 + w2 + w3 + w4 );
}

// six planes (2 maps x 3 channels) of size W*H each, plane stride = W*H
// (planes p0 .. p1 - 1 of the six: all of them, or one per workgroup in the coarse-levels kernel)
__device__ __forceinline__ void pushPullMipPixel( int i, const uint8_t* img, const uint8_t* occ, int W, int H, uint8_t* mip,
                                                  uint8_t* mipOcc, int w, int h, int p0 = 0, int p1 = 6 ) {
  const int  x = i % w, y = i / w, X = 2 * x, Y = 2 * y;
  const bool i2 = X + 1 < W, i3 = Y + 1 < H;
  const int  w1 = occ[size_t( Y ) * W + X] ? 255 : 0;
  const int  w2 = ( i2 && occ[size_t( Y ) * W + X + 1] ) ? 255 : 0;
  const int  w3 = ( i3 && occ[size_t( Y + 1 ) * W + X] ) ? 255 : 0;
  const int  w4 = ( i2 && i3 && occ[size_t( Y + 1 ) * W + X + 1] ) ? 255 : 0;
  const bool any = ( w1 + w2 + w3 + w4 ) > 0;
  mipOcc[i]      = any ? 1 : 0;
  for ( int p = p0; p < p1; ++p ) {
    const uint8_t* s = img + size_t( p ) * W * H;
    uint8_t        v = 0;
    if ( any ) {
      const int v1 = s[size_t( Y ) * W + X], v2 = i2 ? s[size_t( Y ) * W + X + 1] : 0;
      const int v3 = i3 ? s[size_t( Y + 1 ) * W + X] : 0, v4 = ( i2 && i3 ) ? s[size_t( Y + 1 ) * W + X + 1] : 0;
      v            = uint8_t( mean4w( v1, w1, v2, w2, v3, w3, v4, w4 ) );
    }
    mip[size_t( p ) * w * h + i] = v;
  }
}
__global__ __launch_bounds__( 256 ) void pushPullMipKernel( const uint8_t* __restrict__ img, const uint8_t* __restrict__ occ, int W,
                                                             int H, uint8_t* __restrict__ mip, uint8_t* __restrict__ mipOcc, int w,
                                                             int h ) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i < w * h ) pushPullMipPixel( i, img, occ, W, H, mip, mipOcc, w, h );
}

__device__ __forceinline__ void pushPullFillPixel( int i, uint8_t* img, const uint8_t* occ, int W, int H, const uint8_t* mip, int w,
                                                   int h, int p0 = 0, int p1 = 6 ) {
  if ( occ[i] ) return;
  const int  X = i % W, Y = i / W, x = X >> 1, y = Y >> 1;
  const int  dx = ( X & 1 ) ? 1 : -1, dy = ( Y & 1 ) ? 1 : -1;
  const bool hx = dx < 0 ? x > 0 : x < w - 1, hy = dy < 0 ? y > 0 : y < h - 1;
  for ( int p = p0; p < p1; ++p ) {
    const uint8_t* m  = mip + size_t( p ) * w * h;
    const int      v  = m[size_t( y ) * w + x];
    const int      vx = hx ? m[size_t( y ) * w + x + dx] : 0;
    const int      vy = hy ? m[size_t( y + dy ) * w + x] : 0;
    const int      vd = ( hx && hy ) ? m[size_t( y + dy ) * w + x + dx] : 0;
    img[size_t( p ) * W * H + i] = uint8_t( mean4w( v, 144, vx, hx ? 48 : 0, vy, hy ? 48 : 0, vd, ( hx && hy ) ? 16 : 0 ) );
  }
}
__global__ __launch_bounds__( 256 ) void pushPullFillKernel( uint8_t* __restrict__ img, const uint8_t* __restrict__ occ, int W, int H,
                                                              const uint8_t* __restrict__ mip, int w, int h ) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i < W * H ) pushPullFillPixel( i, img, occ, W, H, mip, w, h );
}

__device__ __forceinline__ void pushPullBlurPixel( int i, const uint8_t* src, uint8_t* dst, const uint8_t* occ, int W, int H, int p0 = 0,
                                                   int p1 = 6 ) {
  if ( occ[i] ) return;
  const int x = i % W, y = i / W;
  const int x1 = x > 0 ? x - 1 : x, y1 = y > 0 ? y - 1 : y, x2 = x < W - 1 ? x + 1 : x, y2 = y < H - 1 ? y + 1 : y;
  for ( int p = p0; p < p1; ++p ) {
    const uint8_t* s   = src + size_t( p ) * W * H;
    const int      sum = s[size_t( y1 ) * W + x1] + s[size_t( y1 ) * W + x2] + s[size_t( y2 ) * W + x1] + s[size_t( y2 ) * W + x2] +
                    s[size_t( y ) * W + x1] + s[size_t( y ) * W + x2] + s[size_t( y1 ) * W + x] + s[size_t( y2 ) * W + x];
    dst[size_t( p ) * W * H + i] = uint8_t( ( sum + 4 ) >> 3 );
  }
}
__global__ __launch_bounds__( 256 ) void pushPullBlurKernel( const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const uint8_t* __restrict__ occ, int W, int H ) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i < W * H ) pushPullBlurPixel( i, src, dst, occ, W, H );
}

// ---- S21, packed: a lane works on FOUR horizontally adjacent pixels, one aligned 32-bit LDS word ---------------------------
// Rows lie in LDS with a pitch that is a whole number of words; byte j of word wx of a row is pixel 4 wx + j.  Next to each image
// word lies a mask word, 0xFF in the bytes of the occupied pixels (and of the bytes beyond the row's last pixel): those never
// change.  The eight-neighbour sum is the 3 x 3 box sum less the centre.  The box sum is taken vertically first -- the three rows'
// bytes of a column added in 16-bit fields, pixels 0 and 2 of the word in one register, 1 and 3 in another, the column left of the
// word and the one right of it in a third -- and then horizontally by shifting fields (a sum is at most 9 x 255 + 4).
struct PushPullEdge {  // per lane: where the row's first and last pixel sit, if in this word (the reference's clamp, by selects)
  bool     first;      // pixel 0 of the word is the row's first: its left neighbour is itself
  bool     last3;      // pixel 3 of the word is the row's last: its right neighbour is itself
  uint32_t after;      // the byte after the row's last pixel, if that is pixel 0, 1 or 2 of this word: it repeats the pixel before it
};
__device__ __forceinline__ PushPullEdge pushPullEdge( int wx, int w ) {
  const bool last = wx == ( ( w - 1 ) >> 2 );
  const int  b    = ( w - 1 ) & 3;
  return PushPullEdge{wx == 0, last && b == 3, last && b < 3 ? 0xFF00u << ( 8 * b ) : 0u};
}
struct PushPullRow {
  uint32_t lo, hi, e;  // the bytes of the pixels 0, 2 (lo) and 1, 3 (hi) of a word, and of its neighbours left (low half) and right
};
// l, c, r: the words left of, at and right of the position
__device__ __forceinline__ PushPullRow pushPullRowTerms( uint32_t l, uint32_t c, uint32_t r, const PushPullEdge& E ) {
  constexpr uint32_t kF = 0x00FF00FFu;
  const uint32_t     cp = ( c & ~E.after ) | ( ( c << 8 ) & E.after );
  const uint32_t     lb = E.first ? c & 0xFFu : l >> 24, rb = E.last3 ? c >> 24 : r & 0xFFu;
  return PushPullRow{cp & kF, ( cp >> 8 ) & kF, lb | ( rb << 16 )};
}
// One blur pass over the rows y0 .. y1 - 1 of word column wx: src -> dst (both with a readable word before the first and after the
// last), `rows` rows of `pitch` words.  Walks down with the terms of two rows in registers, R rows at a time: the reads of the R
// rows below -- three words and a mask word each -- are issued together, then R words are computed and written.  Row indices
// clamp at 0 and rows - 1 (offsets are carried, not multiplied).
template <int R>
__device__ __forceinline__ void pushPullBlurStrip( const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                   const uint32_t* __restrict__ occ, int pitch, int rows, int wx, int y0, int y1,
                                                   const PushPullEdge& E ) {
  constexpr uint32_t kF = 0x00FF00FFu;
  const int          oLast = ( rows - 1 ) * pitch + wx;
  int                o = y0 * pitch + wx;
  const uint32_t*    s = src + max( o - pitch, wx );
  PushPullRow        up = pushPullRowTerms( s[-1], s[0], s[1], E );
  s                     = src + o;
  uint32_t    cw  = s[0];
  PushPullRow mid = pushPullRowTerms( s[-1], cw, s[1], E );
  for ( int y = y0; y < y1; y += R ) {
    uint32_t l[R], c[R], r[R], m[R];
    int      at[R];
#pragma unroll
    for ( int k = 0; k < R; ++k ) {
      at[k]               = min( o + k * pitch, oLast );
      const uint32_t* n   = src + min( o + ( k + 1 ) * pitch, oLast );
      l[k] = n[-1], c[k] = n[0], r[k] = n[1], m[k] = occ[at[k]];
    }
#pragma unroll
    // The mask words are used only under `y + k < y1`.  Left alone, the compiler moves each ds_read of a mask into the exec-masked
    // block of its store, behind a wait of its own (seen in the gfx950 assembly: R - 1 further LDS round trips per batch); the pin
    // keeps the R reads with the other reads of the batch (loads.h).  Not timed without it: the passes are bound by their VALU
    // work either way (profiles/attribute_padding.txt, section 3); without it the result is the same.
    for ( int k = 0; k < R; ++k ) pin( m[k] );
#pragma unroll
    for ( int k = 0; k < R; ++k ) {
      const PushPullRow dn  = pushPullRowTerms( l[k], c[k], r[k], E );
      const uint32_t    vlo = up.lo + mid.lo + dn.lo, vhi = up.hi + mid.hi + dn.hi, ve = up.e + mid.e + dn.e, t = vlo + vhi;
      // t = columns (0 + 1, 2 + 3); with columns (-1, 1) the sums around the pixels 0, 2, with columns (2, 4) those around 1, 3
      const uint32_t slo = t + ( ( vhi << 16 ) | ( ve & 0xFFFFu ) ), shi = t + ( ( vlo >> 16 ) | ( ve & 0xFFFF0000u ) );
      const uint32_t lo = ( ( slo - mid.lo + 0x00040004u ) >> 3 ) & kF, hi = ( ( shi - mid.hi + 0x00040004u ) >> 3 ) & kF;
      if ( y + k < y1 ) dst[at[k]] = ( cw & m[k] ) | ( ( lo | ( hi << 8 ) ) & ~m[k] );
      up = mid, mid = dn, cw = c[k];
    }
    o += R * pitch;
  }
}

// pushPullFillPixel's value for pixel (X, Y) from the coarser level m (w x h, rows `pitch` bytes apart).  mean4w's weights are 144,
// 48, 48, 16, or 0 for a neighbour beyond the edge.  With the coordinate of such a neighbour clamped instead -- it then repeats a
// pixel that is there -- the full form gives the same integer quotient: (144 + 48) v + (48 + 16) vy over 256 is 3 v + vy over 4, the
// form with the x neighbour missing, likewise in y, and 256 v over 256 is v.  So: four loads that never leave the level, one shift.
__device__ __forceinline__ uint32_t pushPullFillValue( const uint8_t* m, int pitch, int w, int h, int X, int Y ) {
  const int      x = X >> 1, y = Y >> 1;
  const int      xn = ( X & 1 ) ? min( x + 1, w - 1 ) : max( x - 1, 0 ), yn = ( Y & 1 ) ? min( y + 1, h - 1 ) : max( y - 1, 0 );
  const uint8_t *r0 = m + size_t( y ) * pitch, *r1 = m + size_t( yn ) * pitch;
  return ( 9u * r0[x] + 3u * r0[xn] + 3u * r1[x] + r1[xn] ) >> 4;
}

// four bytes from any address (the rows and planes of the images are not word aligned)
__device__ __forceinline__ uint32_t pushPullLoad4( const uint8_t* p ) {
  uint32_t v;
  __builtin_memcpy( &v, p, 4 );
  return v;
}

// One level of the way up in ONE launch: the fill from the coarser level and all `iters` blur passes, a 96 x 96 tile of one
// plane per workgroup, in LDS.  The tile is loaded with a margin of `iters` pixels (clipped to the image): a blur pass reads
// the 8 neighbours, so pass k (of iters, from 0) is computed on the tile grown by iters - 1 - k pixels only -- what the later
// passes can still carry into the tile -- and reads nothing but what the pass before computed or the load put there.  Coordinates
// clamp at the region's edges, which a pass reaches only where they are the image's edges.  Occupied pixels never change; only
// unoccupied pixels of the tile are written, and no workgroup USES a pixel another one writes: unoccupied pixels are computed
// from the coarser level.  (The word load of four pixels does fetch the bytes of unoccupied pixels, which the tile that owns
// them may be storing at that moment; the byte mask drops them before anything is computed, so whatever they hold -- the clear
// of d_attr, or the other tile's result -- reaches nothing.)  A tile without an unoccupied pixel is left after the load.
constexpr int kPushPullTile = 96, kPushPullSpan = 128, kPushPullMaxIters = ( kPushPullSpan - kPushPullTile ) / 2;
constexpr int kPushPullPitch = kPushPullSpan / 4, kPushPullWords = kPushPullPitch * kPushPullSpan;
// 512 threads: a lane per word column and sixteen strips of rows (256 and 1 024 measured slower, profiles/attribute_padding.txt)
constexpr int kPushPullThreads = 512, kPushPullStrips = kPushPullThreads / kPushPullPitch;
static_assert( kPushPullThreads % kPushPullPitch == 0 && kPushPullThreads <= 1024, "whole strips of word columns" );
__global__ __launch_bounds__( kPushPullThreads ) void pushPullFillBlurKernel( uint8_t* __restrict__ img, const uint8_t* __restrict__ occ,
                                                                               int W, int H, const uint8_t* __restrict__ mip, int w, int h,
                                                                               int iters, int tilesX ) {
  __shared__ uint32_t sOcc[kPushPullWords];
  __shared__ uint32_t sBuf[2 * kPushPullWords + 2];  // (a word before the first buffer and one after the second: the strips' l and r)
  const int      X0 = ( blockIdx.x % tilesX ) * kPushPullTile, Y0 = ( blockIdx.x / tilesX ) * kPushPullTile;
  const int      RX0 = max( X0 - iters, 0 ), RY0 = max( Y0 - iters, 0 );
  const int      RW = min( X0 + kPushPullTile + iters, W ) - RX0, RH = min( Y0 + kPushPullTile + iters, H ) - RY0;
  const int      CX0 = X0 - RX0, CX1 = min( X0 + kPushPullTile, W ) - RX0, CY0 = Y0 - RY0, CY1 = min( Y0 + kPushPullTile, H ) - RY0;
  uint8_t*       plane = img + size_t( blockIdx.y ) * W * H;
  const uint8_t* m     = mip + size_t( blockIdx.y ) * w * h;
  const int      wx = threadIdx.x & ( kPushPullPitch - 1 ), strip = threadIdx.x / kPushPullPitch;
  // The load: a lane keeps its word column.  A word wholly inside the region takes four loads that depend on nothing but the
  // position -- its occupancies, its pixels and the two rows of four coarse pixels its fills can touch (pushPullFillValue), each as one
  // unaligned 32-bit load -- so the rows of a lane are in flight together; the word that holds the region's last pixels, and every
  // word over a coarse level narrower than four pixels, goes pixel by pixel.
  const int      rx0 = 4 * wx, XW = RX0 + rx0, mb = w >= 4 ? min( max( ( XW >> 1 ) - 1, 0 ), w - 4 ) : 0;
  const uint32_t coreX = ( rx0 >= CX0 && rx0 < CX1 ? 0xFFu : 0u ) | ( rx0 + 1 >= CX0 && rx0 + 1 < CX1 ? 0xFF00u : 0u ) |
                         ( rx0 + 2 >= CX0 && rx0 + 2 < CX1 ? 0xFF0000u : 0u ) | ( rx0 + 3 >= CX0 && rx0 + 3 < CX1 ? 0xFF000000u : 0u );
  int            hole  = 0;  // an unoccupied pixel of the tile seen by this lane
  if ( rx0 + 3 < RW && w >= 4 ) {
#pragma unroll 4
    for ( int ry = strip; ry < RH; ry += kPushPullStrips ) {
      const int      Y = RY0 + ry, y = Y >> 1, yn = ( Y & 1 ) ? min( y + 1, h - 1 ) : max( y - 1, 0 );
      const size_t   g  = size_t( Y ) * W + XW;
      const uint32_t o4 = pushPullLoad4( occ + g ), p4 = pushPullLoad4( plane + g );
      const uint32_t r0 = pushPullLoad4( m + size_t( y ) * w + mb ), r1 = pushPullLoad4( m + size_t( yn ) * w + mb );
      const uint32_t nz = ( ( ( o4 & 0x7F7F7F7Fu ) + 0x7F7F7F7Fu ) | o4 ) & 0x80808080u, msk = ( nz >> 7 ) * 0xFFu;
      uint32_t       fill = 0;
#pragma unroll
      for ( int j = 0; j < 4; ++j ) {
        const int      X = XW + j, x = X >> 1, xn = ( X & 1 ) ? min( x + 1, w - 1 ) : max( x - 1, 0 ), sx = 8 * ( x - mb ), sn = 8 * ( xn - mb );
        fill |= ( ( 9u * ( ( r0 >> sx ) & 0xFFu ) + 3u * ( ( r0 >> sn ) & 0xFFu ) + 3u * ( ( r1 >> sx ) & 0xFFu ) + ( ( r1 >> sn ) & 0xFFu ) ) >> 4 ) << ( 8 * j );
      }
      const uint32_t pix = ( p4 & msk ) | ( fill & ~msk );
      const int      i   = ry * kPushPullPitch + wx;
      hole |= int( ( ~msk & coreX ) != 0 && ry >= CY0 && ry < CY1 );
      sOcc[i] = msk, sBuf[1 + i] = pix, sBuf[1 + kPushPullWords + i] = pix;
    }
  } else {
    for ( int ry = strip; ry < RH; ry += kPushPullStrips ) {
      const int Y = RY0 + ry, i = ry * kPushPullPitch + wx;
      uint32_t  pix = 0, msk = 0;
#pragma unroll
      for ( int j = 0; j < 4; ++j ) {
        const int rx = rx0 + j, X = RX0 + rx;
        uint32_t  v = 0, o = 0xFFu;  // beyond the region: a constant
        if ( rx < RW ) {
          const size_t g = size_t( Y ) * W + X;
          o              = occ[g] ? 0xFFu : 0u;
          v              = o ? uint32_t( plane[g] ) : pushPullFillValue( m, w, w, h, X, Y );
          hole |= int( !o && rx >= CX0 && rx < CX1 && ry >= CY0 && ry < CY1 );
        }
        pix |= v << ( 8 * j ), msk |= o << ( 8 * j );
      }
      sOcc[i] = msk, sBuf[1 + i] = pix, sBuf[1 + kPushPullWords + i] = pix;
    }
  }
  if ( !__syncthreads_or( hole ) ) return;
  const PushPullEdge edge = pushPullEdge( wx, RW );
  int            cur = 0;
  for ( int it = 0; it < iters; ++it ) {
    const int g  = iters - 1 - it;
    const int xa = max( X0 - g, 0 ) - RX0, xb = min( X0 + kPushPullTile + g, W ) - RX0;
    const int ya = max( Y0 - g, 0 ) - RY0, yb = min( Y0 + kPushPullTile + g, H ) - RY0;
    const int per = ( yb - ya + kPushPullStrips - 1 ) / kPushPullStrips, y0 = ya + strip * per, y1 = min( y0 + per, yb );
    if ( wx >= ( xa >> 2 ) && wx <= ( ( xb - 1 ) >> 2 ) && y0 < y1 )
      pushPullBlurStrip<4>( sBuf + 1 + cur * kPushPullWords, sBuf + 1 + ( cur ^ 1 ) * kPushPullWords, sOcc, kPushPullPitch, RH, wx, y0, y1,
                            edge );
    __syncthreads();
    cur ^= 1;
  }
  const uint32_t* res = sBuf + 1 + cur * kPushPullWords;
  for ( int i = kPushPullPitch * CY0 + threadIdx.x; i < kPushPullPitch * CY1; i += kPushPullThreads ) {
    const int      cx = i & ( kPushPullPitch - 1 ), ry = i / kPushPullPitch;
    const uint32_t v = res[i], o = sOcc[i];
#pragma unroll
    for ( int j = 0; j < 4; ++j ) {
      const int rx = 4 * cx + j;
      if ( rx >= CX0 && rx < CX1 && !( ( o >> ( 8 * j ) ) & 0xFFu ) ) plane[size_t( RY0 + ry ) * W + RX0 + rx] = uint8_t( v >> ( 8 * j ) );
    }
  }
}

// The coarse end of the pyramid in ONE workgroup per plane, in LDS: the levels from the first of at most kPushPullSmall pixels down
// -- their mip maps on the way down, and on the way up the fill and the 4, 5, ... blur iterations of every level.  Level `first`
// (made by the launch before) is read from global memory once; every step after that works on LDS, a workgroup barrier between
// two steps; only the final image of level `first` goes back, into the buffer of the level the host's parity rule names (nothing
// outside this kernel reads the coarser levels or their occupancies).  Every level keeps its image, its ping-pong partner and its
// mask in words (pushPullBlurStrip); the fill writes both partners, which is the copy the separate launches made.
constexpr int kPushPullSmall  = 160 * 160;
constexpr int kPushPullLevels = 16;
struct PushPullLevels {
  int            count;  // levels of the pyramid, 0 = the canvas
  int            first;  // the first (finest) level handled here
  int            w[kPushPullLevels], h[kPushPullLevels];
  const uint8_t *img, *occ;  // level `first`: six planes, one occupancy
  uint8_t*       out;        // level `first` after its blur passes: six planes
};
// words of LDS a level takes: a word in front, image, partner, a word behind, mask
__host__ __device__ inline int pushPullLevelWords( int w, int h ) { return 3 * ( ( w + 3 ) >> 2 ) * h + 2; }
__global__ __launch_bounds__( 1024 ) void pushPullCoarseLevelsKernel( PushPullLevels L ) {
  extern __shared__ uint32_t sPyr[];
  // The six planes (2 maps x 3 channels) never read each other: one workgroup per plane.  The occupancy of the coarse levels is
  // common to the planes: every workgroup derives it for itself.
  const int plane = int( blockIdx.x ), tid = int( threadIdx.x );
  int       w = L.w[L.first], h = L.h[L.first], pw = ( w + 3 ) >> 2, n = pw * h, base = 0;
  {
    const uint8_t* src = L.img + size_t( plane ) * w * h;
    uint32_t *     img = sPyr + base + 1, *occ = sPyr + base + 2 + 2 * n;
    for ( int i = tid; i < n; i += 1024 ) {
      const int wx = i % pw, y = i / pw;
      uint32_t  pix = 0, msk = 0;
#pragma unroll
      for ( int j = 0; j < 4; ++j ) {
        const int x = 4 * wx + j;
        uint32_t  v = 0, o = 0xFFu;
        if ( x < w ) {
          const size_t g = size_t( y ) * w + x;
          o = L.occ[g] ? 0xFFu : 0u, v = src[g];
        }
        pix |= v << ( 8 * j ), msk |= o << ( 8 * j );
      }
      img[i] = pix, occ[i] = msk;
    }
  }
  __syncthreads();
  // down: mip maps of the levels first + 1 .. count - 1 (pushPullMipPixel; mean4w with weights of 255 or 0 is the sum of the
  // occupied pixels over their number)
  for ( int l = L.first + 1; l < L.count; ++l ) {
    const int      W = w, H = h, fp = 4 * pw;
    const uint8_t *fimg = reinterpret_cast<const uint8_t*>( sPyr + base + 1 ), *focc = reinterpret_cast<const uint8_t*>( sPyr + base + 2 + 2 * n );
    base += 3 * n + 2;
    w = L.w[l], h = L.h[l], pw = ( w + 3 ) >> 2, n = pw * h;
    uint32_t *img = sPyr + base + 1, *occ = sPyr + base + 2 + 2 * n;
    for ( int i = tid; i < n; i += 1024 ) {
      const int wx = i % pw, y = i / pw, Y = 2 * y;
      uint32_t  pix = 0, msk = 0;
#pragma unroll
      for ( int j = 0; j < 4; ++j ) {
        const int x = 4 * wx + j, X = 2 * x;
        uint32_t  v = 0, o = 0xFFu;
        if ( x < w ) {
          const bool i2 = X + 1 < W, i3 = Y + 1 < H;
          const int  a = Y * fp + X;
          const bool o1 = focc[a], o2 = i2 && focc[a + 1], o3 = i3 && focc[a + fp], o4 = i2 && i3 && focc[a + fp + 1];
          const int  cnt = int( o1 ) + int( o2 ) + int( o3 ) + int( o4 );
          const int  sum = ( o1 ? fimg[a] : 0 ) + ( o2 ? fimg[a + 1] : 0 ) + ( o3 ? fimg[a + fp] : 0 ) + ( o4 ? fimg[a + fp + 1] : 0 );
          o              = cnt ? 0xFFu : 0u;
          v              = cnt == 3 ? uint32_t( sum ) / 3u : uint32_t( sum ) >> ( cnt >> 1 );
        }
        pix |= v << ( 8 * j ), msk |= o << ( 8 * j );
      }
      img[i] = pix, occ[i] = msk;
    }
    __syncthreads();
  }
  // up: fill level l - 1 from level l, then iters blur passes between the level's two buffers (host loop of
  // generateAttributeImages, same order); an odd count leaves the level's image in the partner
  int iters = 4, inTmp = 0;
  for ( int l = L.count - 1; l > L.first; --l ) {
    const int      cw = w, ch = h, cp = 4 * pw;
    const uint8_t* m = reinterpret_cast<const uint8_t*>( sPyr + base + 1 + ( inTmp ? n : 0 ) );
    w = L.w[l - 1], h = L.h[l - 1], pw = ( w + 3 ) >> 2, n = pw * h;
    base -= 3 * n + 2;
    uint32_t *      img = sPyr + base + 1, *tmp = img + n;
    const uint32_t* occ = sPyr + base + 2 + 2 * n;
    for ( int i = tid; i < n; i += 1024 ) {
      const int      wx = i % pw, y = i / pw;
      const uint32_t msk = occ[i];
      uint32_t       pix = img[i];
#pragma unroll
      for ( int j = 0; j < 4; ++j )
        if ( !( ( msk >> ( 8 * j ) ) & 0xFFu ) ) pix = ( pix & ~( 0xFFu << ( 8 * j ) ) ) | ( pushPullFillValue( m, cp, cw, ch, 4 * wx + j, y ) << ( 8 * j ) );
      img[i] = pix, tmp[i] = pix;
    }
    __syncthreads();
    // strips of `per` rows, as many as give every lane one while the rows last
    const int per = ( h + max( 1024 / pw, 1 ) - 1 ) / max( 1024 / pw, 1 ), strips = ( h + per - 1 ) / per;
    for ( int it = 0; it < iters; ++it ) {
      const uint32_t* src = ( it & 1 ) ? tmp : img;
      uint32_t*       dst = ( it & 1 ) ? img : tmp;
      for ( int i = tid; i < pw * strips; i += 1024 ) {
        const int wx = i % pw, y0 = ( i / pw ) * per;
        pushPullBlurStrip<2>( src, dst, occ, pw, h, wx, y0, min( y0 + per, h ), pushPullEdge( wx, w ) );
      }
      __syncthreads();
    }
    inTmp = iters & 1;
    iters = min( iters + 1, 16 );
  }
  {
    const uint32_t* res = sPyr + base + 1 + ( inTmp ? n : 0 );
    uint8_t*        out = L.out + size_t( plane ) * w * h;
    for ( int i = tid; i < n; i += 1024 ) {
      const int      wx = i % pw, y = i / pw;
      const uint32_t v = res[i];
#pragma unroll
      for ( int j = 0; j < 4; ++j )
        if ( 4 * wx + j < w ) out[size_t( y ) * w + 4 * wx + j] = uint8_t( v >> ( 8 * j ) );
    }
  }
}

// ---- S22 ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__( 256 ) void attributeGroupDilateKernel( const uint8_t* __restrict__ occ, int W, int H,
                                                                      uint8_t* __restrict__ attr ) {
  const size_t c = size_t( blockIdx.x ) * blockDim.x + threadIdx.x, plane = size_t( W ) * H;
  if ( c >= plane || occ[c] ) return;
#pragma unroll
  for ( int k = 0; k < 3; ++k ) {
    const uint32_t a = attr[k * plane + c], b = attr[( 3 + k ) * plane + c];
    const uint8_t  v = uint8_t( ( a + b + 1 ) >> 1 );
    attr[k * plane + c] = attr[( 3 + k ) * plane + c] = v;
  }
}

}  // namespace

// S18 off the CTC point (the caller has checked the set against both clouds).  Device memory held: the forward rows
// M x width( kFwd ) and the backward rows n x width( kBwd ) of (index, distance), the n x kBwd backward entries of 8 bytes, and per
// target three words and the forward colour.
static int transferColorsRules( tmc2_ctx* ctx, const TreeDev& srcTree, const Pt* d_srcPts, const uint8_t* d_srcRgb4, uint32_t n,
                                const TreeDev& tgtTree, const Pt* d_tgtPts, uint32_t M, uint8_t* d_outRgb4, uint32_t* d_error,
                                const CtRules& p ) {
  hipStream_t      s = ctx->stream;
  const dim3       blk( 256 );
  const int        wf = knnWidth( p.kFwd ), wb = knnWidth( p.kBwd );
  DevBuf<uint32_t> d_idxF, d_distF, d_easyF, d_idxB, d_distB, d_count, d_offset, d_cursor;
  DevBuf<uint2>    d_entries;
  DevBuf<uint8_t>  d_fwd;
  TMC2_TRY( d_idxF.alloc( size_t( M ) * wf ) );
  TMC2_TRY( d_distF.alloc( size_t( M ) * wf ) );
  TMC2_TRY( d_idxB.alloc( size_t( n ) * wb ) );
  TMC2_TRY( d_distB.alloc( size_t( n ) * wb ) );
  TMC2_TRY( d_count.alloc( M ) );
  TMC2_TRY( d_offset.alloc( M ) );
  TMC2_TRY( d_cursor.alloc( M ) );
  TMC2_TRY( d_entries.alloc( size_t( n ) * p.kBwd ) );
  TMC2_TRY( d_fwd.alloc( size_t( M ) * 4 ) );
  // The split form answers a query that has an identical point with one descent: forward only where that point's colour is all
  // the rule reads (the skip flag), backward only at one result; otherwise the whole list is needed.
  if ( p.skipFwd ) {
    TMC2_TRY( d_easyF.alloc( M ) );
    TMC2_TRY( launchKnnSplit( ctx, srcTree, d_tgtPts, M, wf, d_easyF.p, d_idxF.p, d_distF.p, "knn_recon_in_source", false, p.kFwd ) );
  } else {
    TMC2_TRY( launchKnnTree( ctx, srcTree, d_tgtPts, M, wf, d_idxF.p, d_distF.p, "knn_recon_in_source", p.kFwd ) );
  }
  if ( p.kBwd == 1 )
    TMC2_TRY( launchKnnSplit( ctx, tgtTree, d_srcPts, n, 1, d_idxB.p, d_idxB.p, d_distB.p, "knn_source_in_recon" ) );
  else
    TMC2_TRY( launchKnnTree( ctx, tgtTree, d_srcPts, n, wb, d_idxB.p, d_distB.p, "knn_source_in_recon", p.kBwd ) );
  StageScope stage( ctx, "transfer_colors" );
  TMC2_TRY( fillRegions( ctx, {{d_count.p, size_t( M ) * 4, 0}, {d_cursor.p, size_t( M ) * 4, 0}, {d_error, 4, 0}} ) );
  const dim3 grdM( ( M + 255 ) / 256 ), grdN( ( n + 255 ) / 256 );
  hipLaunchKernelGGL( forwardColorRulesKernel, grdM, blk, 0, s, d_idxF.p, d_distF.p, wf, p.skipFwd ? d_easyF.p : (const uint32_t*)nullptr,
                      d_srcRgb4, M, p, d_fwd.p );
  hipLaunchKernelGGL( backwardVoteRulesKernel<false>, grdN, blk, 0, s, d_idxB.p, d_distB.p, wb, n, p.kBwd, p.geoBwd, d_count.p, d_offset.p,
                      d_entries.p );
  TMC2_TRY( exclusiveScanU32( ctx, d_count.p, d_offset.p, M, nullptr ) );
  hipLaunchKernelGGL( backwardVoteRulesKernel<true>, grdN, blk, 0, s, d_idxB.p, d_distB.p, wb, n, p.kBwd, p.geoBwd, d_cursor.p, d_offset.p,
                      d_entries.p );
  hipLaunchKernelGGL( combineColorRulesKernel, grdM, blk, 0, s, d_count.p, d_offset.p, d_entries.p, d_srcRgb4, d_fwd.p, M, p,
                      1.0 / double( M ), 1.0 / double( n ), d_outRgb4, d_error );
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;
}

// S18 on device-resident clouds: source (tree + original-order points + colours) -> target (tree + points).  params: nullptr or a
// checked set; the CTC point (ctIsDefault) runs the kernels written for it, every other set the rules over its own lists.
int transferColorsDevice( tmc2_ctx* ctx, const TreeDev& srcTree, const Pt* d_srcPts, const uint8_t* d_srcRgb4, uint32_t n,
                          const TreeDev& tgtTree, const Pt* d_tgtPts, uint32_t M, uint8_t* d_outRgb4, uint32_t* d_error,
                          const tmc2_color_transfer_params* params = nullptr ) {
  // (option COLOR_TRANSFER_RULES=1: the rules kernels at the CTC point too -- what pins the two texts of one rule to each other)
  const auto forced = ctxOption( ctx, "COLOR_TRANSFER_RULES" );
  if ( params && ( !ctIsDefault( *params ) || ( forced && ( *forced )[0] == '1' ) ) )
    return transferColorsRules( ctx, srcTree, d_srcPts, d_srcRgb4, n, tgtTree, d_tgtPts, M, d_outRgb4, d_error, ctRules( *params ) );
  hipStream_t      s = ctx->stream;
  const dim3       blk( 256 );
  DevBuf<uint32_t> d_idx8, d_dist8, d_idx1, d_dist1, d_count, d_offset, d_cursor;
  DevBuf<uint2>    d_entries;
  DevBuf<uint8_t>  d_fwd;
  TMC2_TRY( d_idx8.alloc( size_t( M ) * 8 ) );
  TMC2_TRY( d_dist8.alloc( size_t( M ) * 8 ) );
  TMC2_TRY( d_idx1.alloc( n ) );
  TMC2_TRY( d_dist1.alloc( n ) );
  TMC2_TRY( d_count.alloc( M ) );
  TMC2_TRY( d_offset.alloc( M ) );
  TMC2_TRY( d_cursor.alloc( M ) );
  TMC2_TRY( d_entries.alloc( n ) );
  TMC2_TRY( d_fwd.alloc( size_t( M ) * 4 ) );
  // (round 6: both searches in two launches -- the queries that have an identical point in the tree first, then the compacted
  //  rest: knn.hip, launchKnnSplit; the one-launch form of rounds 1-5 was removed)
  DevBuf<uint32_t> d_easy8;
  TMC2_TRY( d_easy8.alloc( M ) );
  TMC2_TRY( launchKnnSplit( ctx, srcTree, d_tgtPts, M, 8, d_easy8.p, d_idx8.p, d_dist8.p, "knn8_recon_in_source" ) );
  TMC2_TRY( launchKnnSplit( ctx, tgtTree, d_srcPts, n, 1, d_idx1.p, d_idx1.p, d_dist1.p, "knn1_source_in_recon" ) );
  StageScope stage( ctx, "transfer_colors" );
  TMC2_TRY( fillRegions( ctx, {{d_count.p, size_t( M ) * 4, 0}, {d_cursor.p, size_t( M ) * 4, 0}, {d_error, 4, 0}} ) );
  const dim3 grdM( ( M + 255 ) / 256 ), grdN( ( n + 255 ) / 256 );
  hipLaunchKernelGGL( forwardColorKernel, grdM, blk, 0, s, d_idx8.p, d_dist8.p, d_easy8.p, d_srcRgb4, M, d_fwd.p );
  hipLaunchKernelGGL( backwardVoteKernel<false>, grdN, blk, 0, s, d_idx1.p, d_dist1.p, n, d_count.p, d_offset.p, d_entries.p );
  TMC2_TRY( exclusiveScanU32( ctx, d_count.p, d_offset.p, M, nullptr ) );
  hipLaunchKernelGGL( backwardVoteKernel<true>, grdN, blk, 0, s, d_idx1.p, d_dist1.p, n, d_cursor.p, d_offset.p, d_entries.p );
  hipLaunchKernelGGL( combineColorKernel, grdM, blk, 0, s, d_count.p, d_offset.p, d_entries.p, d_srcRgb4, d_fwd.p, M,
                      d_outRgb4, d_error );
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;
}

// S17 + the k-d tree over the reconstruction: all the decoder needs before the post-reconstruction tail, and the first half
// of the encoder's phase B
int reconstructPointCloud( tmc2_frame* f, const PbfParams* pbfParams ) {
  if ( !f->haveGeometryImages ) {
    setError( "generatePointCloud: geometry images missing" );
    return TMC2_E_STATE;
  }
  if ( pbfParams ) {  // (refused before the frame's state changes and before anything is launched)
    if ( const char* what = pbfRefusal( f->occPrecision, *pbfParams, long( f->patches.size() ) ) ) {
      setError( "generatePointCloud (patch border filtering): unsupported %s", what );
      return TMC2_E_UNSUPPORTED;
    }
  }
  // the attribute images are the encoder's product of the plain reconstruction: a reconstruction with occupancy synthesis (the
  // decoder-side leg of such a stream) and the plain one that undoes it leave them standing
  const bool keepAttributeImages = f->haveAttributeImages && ( pbfParams || f->havePbf );
  f->canvasesChanged();  // (the reconstruction is about to be replaced: what is derived from the canvases starts over)
  f->haveAttributeImages = keepAttributeImages;
  if ( pbfParams ) TMC2_TRY( patchBorderFilterDevice( f, *pbfParams ) );  // (refuses before anything is launched)
  PbfMapsDev pbf;
  if ( pbfParams ) pbf = PbfMapsDev{f->d_pbfOffset.p, f->pbfOcc, f->pbfFlag, f->pbfBorderWidth, nullptr};
  tmc2_ctx*    ctx = f->ctx;
  hipStream_t  s   = ctx->stream;
  const int    W = f->canvasW, H = f->canvasH, prec = f->occPrecision;
  const dim3   blk( 256 );
  const uint32_t tiles = f->tileCount;
  // ---- S17 ----------------------------------------------------------------------------------------------
  StageScope       stage( ctx, "reconstruct" );
  DevBuf<uint32_t> d_tileCount, d_tileOffset, d_small;
  TMC2_TRY( d_tileCount.alloc( std::max( tiles, 1u ) ) );
  TMC2_TRY( d_tileOffset.alloc( std::max( tiles, 1u ) ) );
  TMC2_TRY( d_small.alloc( 8 ) );
  uint32_t M = 0;
  if ( tiles ) {
    if ( pbfParams )
      hipLaunchKernelGGL( ( reconTileKernel<false, true> ), dim3( tiles ), blk, 0, s, f->d_place.p, f->d_tilePatch.p, f->d_occVideo.p,
                          f->d_blockToPatch.p, f->d_geo.p, W, H, prec, d_tileCount.p, (const uint32_t*)nullptr, (Pt*)nullptr,
                          (uint32_t*)nullptr, pbf );
    else
      hipLaunchKernelGGL( reconTileKernel<false>, dim3( tiles ), blk, 0, s, f->d_place.p, f->d_tilePatch.p, f->d_occVideo.p,
                          f->d_blockToPatch.p, f->d_geo.p, W, H, prec, d_tileCount.p, (const uint32_t*)nullptr, (Pt*)nullptr,
                          (uint32_t*)nullptr, PbfMapsDev() );
    volatile uint32_t* answer = ctx->answerLine( tmc2_ctx::kAnswerRecon );  // (the point count straight to a page-locked word: no copy)
    TMC2_TRY( exclusiveScanU32( ctx, d_tileCount.p, d_tileOffset.p, tiles, d_small.p, ScanAnswer{answer, nullptr, 0} ) );
    TMC2_HIP( hipStreamSynchronize( s ) );
    M = answer[0];
  }
  if ( M == 0 && pbfParams ) {
    // the filter may remove every pixel (isolated ones have no 4-neighbour): the reference then reconstructs no point.  The frame
    // has its maps and an empty reconstruction; the tail's stages refuse it (needReconstruction).
    stage.end();
    f->reconCount         = 0;
    f->haveReconstruction = true;
    f->haveBoundaryTypes  = true;
    return TMC2_OK;
  }
  if ( M == 0 ) {
    setError( "generatePointCloud: empty reconstruction" );
    return TMC2_E_STATE;
  }
  TMC2_TRY( f->d_recon.alloc( M ) );
  TMC2_TRY( f->d_pointToPixel.alloc( M ) );
  if ( pbfParams ) {
    // the boundary types come with the points; a copy stays for tmc2_codec_identify_boundary_points to restore them from
    TMC2_TRY( f->d_boundaryType.alloc( M ) );
    TMC2_TRY( f->d_pbfBoundary.alloc( M ) );
    pbf.btype = f->d_boundaryType.p;
    hipLaunchKernelGGL( ( reconTileKernel<true, true> ), dim3( tiles ), blk, 0, s, f->d_place.p, f->d_tilePatch.p, f->d_occVideo.p,
                        f->d_blockToPatch.p, f->d_geo.p, W, H, prec, d_tileCount.p, d_tileOffset.p, f->d_recon.p, f->d_pointToPixel.p,
                        pbf );
    TMC2_HIP( hipMemcpyAsync( f->d_pbfBoundary.p, f->d_boundaryType.p, M, hipMemcpyDeviceToDevice, s ) );
  } else {
    hipLaunchKernelGGL( reconTileKernel<true>, dim3( tiles ), blk, 0, s, f->d_place.p, f->d_tilePatch.p, f->d_occVideo.p,
                        f->d_blockToPatch.p, f->d_geo.p, W, H, prec, d_tileCount.p, d_tileOffset.p, f->d_recon.p,
                        f->d_pointToPixel.p, PbfMapsDev() );
  }
  stage.end();
  f->reconCount = M;
  // ---- tree over the reconstruction (like S1) --------------------------------------------------------------
  TMC2_TRY( buildKdTreePlaced( ctx, f->d_recon.p, M, nullptr, "kdtree_build_recon", f->reconTree ) );
  f->haveReconstruction = true;
  f->haveBoundaryTypes  = pbfParams != nullptr;
  return TMC2_OK;
}

// the number of points reconstructPointCloud( f ) would give, from the resident canvases, with the frame left as it is
static int reconstructionSize( tmc2_frame* f, uint32_t* M ) {
  tmc2_ctx*      ctx   = f->ctx;
  const uint32_t tiles = f->tileCount;
  *M                   = 0;
  if ( !tiles ) return TMC2_OK;
  DevBuf<uint32_t> d_tileCount, d_tileOffset, d_small;
  TMC2_TRY( d_tileCount.alloc( tiles ) );
  TMC2_TRY( d_tileOffset.alloc( tiles ) );
  TMC2_TRY( d_small.alloc( 8 ) );
  hipLaunchKernelGGL( reconTileKernel<false>, dim3( tiles ), dim3( 256 ), 0, ctx->stream, f->d_place.p, f->d_tilePatch.p, f->d_occVideo.p,
                      f->d_blockToPatch.p, f->d_geo.p, f->canvasW, f->canvasH, f->occPrecision, d_tileCount.p, (const uint32_t*)nullptr,
                      (Pt*)nullptr, (uint32_t*)nullptr, PbfMapsDev() );
  volatile uint32_t* answer = ctx->answerLine( tmc2_ctx::kAnswerRecon );
  TMC2_TRY( exclusiveScanU32( ctx, d_tileCount.p, d_tileOffset.p, tiles, d_small.p, ScanAnswer{answer, nullptr, 0} ) );
  TMC2_HIP( hipStreamSynchronize( ctx->stream ) );
  *M = answer[0];
  return TMC2_OK;
}

int generateAttributeImages( tmc2_frame* f, const tmc2_color_transfer_params* params ) {
  if ( !f->haveGeometryImages ) {
    setError( "generateAttributeImages: geometry images missing" );
    return TMC2_E_STATE;
  }
  if ( f->d_rgb.count == 0 ) {
    setError( "generateAttributeImages: the frame has no colours" );
    return TMC2_E_STATE;
  }
  // (refused before the frame's state changes.  A backward neighbour count above 1 is held against the size of the reconstruction
  //  that does not exist yet: the tiles are counted first, on their own -- one launch and a scan, for such sets only)
  if ( params ) {
    TMC2_TRY( checkColorTransferParams( "generateAttributeImages", params, f->n, 0 ) );
    if ( params->numNeighborsColorTransferBwd > 1 ) {
      uint32_t size = 0;
      TMC2_TRY( reconstructionSize( f, &size ) );
      if ( size ) TMC2_TRY( checkColorTransferParams( "generateAttributeImages", params, f->n, size ) );
    }
  }
  TMC2_TRY( f->ensureTree() );
  TMC2_TRY( reconstructPointCloud( f ) );
  tmc2_ctx*    ctx = f->ctx;
  hipStream_t  s   = ctx->stream;
  const int    W = f->canvasW, H = f->canvasH, prec = f->occPrecision;
  const size_t area = size_t( W ) * H;
  const dim3   blk( 256 );
  const uint32_t n = uint32_t( f->n ), M = uint32_t( f->reconCount );
  DevBuf<uint32_t> d_small;
  TMC2_TRY( d_small.alloc( 8 ) );
  // ---- S18 ----------------------------------------------------------------------------------------------
  TMC2_TRY( f->d_reconRgb.alloc( size_t( M ) * 4 ) );
  const dim3 grdM( ( M + 255 ) / 256 );
  // (the sort-depth flag is a page-locked word of the context, read after the stage's last synchronisation: no copy)
  volatile uint32_t* h_err = ctx->answerLine( tmc2_ctx::kAnswerAttrError );
  // (each tree is queried with the other cloud's points: non-negative and below 2^13, like its own)
  TMC2_TRY( transferColorsDevice( ctx, f->tree.view( QueryBox::Tight ), f->d_pts.p, f->d_rgb.p, n, f->reconTree.view( QueryBox::Tight ),
                                  f->d_recon.p, M, f->d_reconRgb.p, const_cast<uint32_t*>( h_err ), params ) );
  // ---- S20 ----------------------------------------------------------------------------------------------
  StageScope      stage( ctx, "attribute_images" );
  DevBuf<uint8_t> d_occ;
  TMC2_TRY( d_occ.alloc( area ) );
  TMC2_TRY( f->d_attr.alloc( 6 * area ) );
  TMC2_HIP( hipMemsetAsync( f->d_attr.p, 0, 6 * area, s ) );
  hipLaunchKernelGGL( upsampleOccupancyKernel, dim3( uint32_t( ( area + 255 ) / 256 ) ), blk, 0, s, f->d_occVideo.p, W, H, prec,
                      d_occ.p );
  hipLaunchKernelGGL( attributeScatterKernel, grdM, blk, 0, s, f->d_reconRgb.p, f->d_pointToPixel.p, M, W, H, f->d_attr.p );
  // ---- S21: pyramid ------------------------------------------------------------------------------------------
  struct Level {
    int      w, h;
    uint8_t *img, *tmp, *occ;
  };
  std::vector<Level> lv;
  lv.push_back( Level{W, H, f->d_attr.p, nullptr, d_occ.p} );
  size_t pyramidBytes = 6 * area;  // ping-pong partner of level 0
  {
    int w = W, h = H;
    for ( ;; ) {
      w = ( w + 1 ) >> 1;
      h = ( h + 1 ) >> 1;
      lv.push_back( Level{w, h, nullptr, nullptr, nullptr} );
      pyramidBytes += size_t( w ) * h * ( 6 + 6 + 1 );
      if ( w <= 4 || h <= 4 ) break;
    }
  }
  DevBuf<uint8_t> d_pyr;
  TMC2_TRY( d_pyr.alloc( pyramidBytes + 64 * lv.size() ) );
  {
    uint8_t* p = d_pyr.p;
    lv[0].tmp  = p;
    p += 6 * area;
    for ( size_t l = 1; l < lv.size(); ++l ) {
      const size_t a = size_t( lv[l].w ) * lv[l].h;
      lv[l].img = p, p += 6 * a;
      lv[l].tmp = p, p += 6 * a;
      lv[l].occ = p, p += ( a + 15 ) & ~size_t( 15 );
    }
  }
  // the coarse end of the pyramid (levels of at most kPushPullSmall pixels) goes through ONE launch, in LDS: from the first
  // level that is small and fits with everything below it (by the rows' word pitch a narrow level takes up to 8 bytes for 5 pixels)
  size_t                firstSmall = lv.size(), coarseLds = 0;
  constexpr size_t      kCoarseLdsMax = 160 * 1024 - 64;  // (allowLargeLds)
  std::vector<size_t>   ldsFrom( lv.size() + 1, 0 );      // bytes of LDS of the levels l .. count - 1
  for ( size_t l = lv.size(); l-- > 1; ) ldsFrom[l] = ldsFrom[l + 1] + sizeof( uint32_t ) * size_t( pushPullLevelWords( lv[l].w, lv[l].h ) );
  if ( lv.size() <= size_t( kPushPullLevels ) )
    for ( size_t l = 1; l < lv.size(); ++l )
      if ( lv[l].w * lv[l].h <= kPushPullSmall && ldsFrom[l] <= kCoarseLdsMax ) {
        firstSmall = l, coarseLds = ldsFrom[l];
        break;
      }
  for ( size_t l = 1; l < lv.size() && l <= firstSmall; ++l ) {
    const int cnt = lv[l].w * lv[l].h;
    hipLaunchKernelGGL( pushPullMipKernel, dim3( ( cnt + 255 ) / 256 ), blk, 0, s, lv[l - 1].img, lv[l - 1].occ, lv[l - 1].w,
                        lv[l - 1].h, lv[l].img, lv[l].occ, lv[l].w, lv[l].h );
  }
  int iters = 4;
  if ( firstSmall + 1 < lv.size() ) {
    PushPullLevels L;
    L.count = int( lv.size() ), L.first = int( firstSmall );
    for ( size_t l = 0; l < lv.size(); ++l ) L.w[l] = lv[l].w, L.h[l] = lv[l].h;
    L.img = lv[firstSmall].img, L.occ = lv[firstSmall].occ;
    for ( size_t l = lv.size() - 1; l > firstSmall; --l ) {  // (an odd iteration count leaves a level's image in its partner buffer)
      if ( iters & 1 ) std::swap( lv[l - 1].img, lv[l - 1].tmp );
      iters = std::min( iters + 1, 16 );
    }
    L.out = lv[firstSmall].img;  // (of the levels the kernel fills, only this one is read again: by the fill of level first - 1)
    if ( coarseLds > 48 * 1024 )
      TMC2_TRY( allowLargeLds( reinterpret_cast<const void*>( pushPullCoarseLevelsKernel ), coarseLds, ctx->device ) );
    hipLaunchKernelGGL( pushPullCoarseLevelsKernel, dim3( 6 ), dim3( 1024 ), coarseLds, s, L );
  }
  for ( size_t l = std::min( firstSmall, lv.size() - 1 ); l >= 1; --l ) {
    Level&    fine = lv[l - 1];
    const int cnt  = fine.w * fine.h;
    const dim3 grd( ( cnt + 255 ) / 256 );
    if ( iters <= kPushPullMaxIters ) {  // fill + every blur pass of the level: one launch, tiles in LDS
      const int tilesX = ( fine.w + kPushPullTile - 1 ) / kPushPullTile, tilesY = ( fine.h + kPushPullTile - 1 ) / kPushPullTile;
      hipLaunchKernelGGL( pushPullFillBlurKernel, dim3( tilesX * tilesY, 6 ), dim3( kPushPullThreads ), 0, s, fine.img, fine.occ, fine.w, fine.h,
                          lv[l].img, lv[l].w, lv[l].h, iters, tilesX );
      iters = std::min( iters + 1, 16 );
      continue;
    }
    hipLaunchKernelGGL( pushPullFillKernel, grd, blk, 0, s, fine.img, fine.occ, fine.w, fine.h, lv[l].img, lv[l].w, lv[l].h );
    TMC2_HIP( hipMemcpyAsync( fine.tmp, fine.img, size_t( 6 ) * cnt, hipMemcpyDeviceToDevice, s ) );
    uint8_t *src = fine.img, *dst = fine.tmp;
    for ( int it = 0; it < iters; ++it ) {
      hipLaunchKernelGGL( pushPullBlurKernel, grd, blk, 0, s, src, dst, fine.occ, fine.w, fine.h );
      std::swap( src, dst );
    }
    if ( src != fine.img ) {  // odd iteration count: latest result sits in the partner buffer
      if ( l - 1 == 0 )
        TMC2_HIP( hipMemcpyAsync( fine.img, src, size_t( 6 ) * cnt, hipMemcpyDeviceToDevice, s ) );
      else
        std::swap( fine.img, fine.tmp );
    }
    iters = std::min( iters + 1, 16 );
  }
  // ---- S22 ----------------------------------------------------------------------------------------------
  hipLaunchKernelGGL( attributeGroupDilateKernel, dim3( uint32_t( ( area + 255 ) / 256 ) ), blk, 0, s, d_occ.p, W, H, f->d_attr.p );
  stage.end();  // (before the host waits: an event recorded after the wait is stamped later)
  TMC2_HIP( hipStreamSynchronize( s ) );
  TMC2_HIP( hipGetLastError() );
  const uint32_t err = *h_err;
  if ( err ) {
    setError( "transferColors: a backward candidate list hit std::sort's depth limit (heapsort fallback of libstdc++ "
              "introsort is not reproduced)" );
    return TMC2_E_UNSUPPORTED;
  }
  f->haveAttributeImages = true;
  return TMC2_OK;
}

}  // namespace tmc2

extern "C" {

// replaces PCCPointSet3::transferColors on two host clouds; rgb out = uint8[m][3]
int tmc2_transfer_colors_ex( tmc2_ctx* ctx, const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n, const int16_t* tgtXyz, uint64_t m,
                             const tmc2_color_transfer_params* params, uint8_t* tgtRgb ) {
  using namespace tmc2;
  if ( !ctx || !srcXyz || !srcRgb || !tgtXyz || !tgtRgb || n < 1 || m < 1 || n > 0x3FFFFFFull || m > 0x7FFFFFF0ull ) {
    setError( "transfer_colors: invalid argument" );
    return TMC2_E_INVALID;
  }
  TMC2_TRY( checkColorTransferParams( "transfer_colors", params, n, m ) );
  ApiScope    scope( ctx );
  hipStream_t s = ctx->stream;
  struct Side {
    DevBuf<Pt> pts;
    DeviceTree tree;
  } S, T;
  auto upload = [&]( Side& sd, const int16_t* xyz, uint64_t cnt ) -> int {
    std::vector<Pt> pts( cnt );
    for ( uint64_t i = 0; i < cnt; ++i ) pts[i] = Pt{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0};
    TMC2_TRY( sd.pts.alloc( cnt ) );
    TMC2_HIP( hipMemcpyAsync( sd.pts.p, pts.data(), cnt * sizeof( Pt ), hipMemcpyHostToDevice, s ) );
    TMC2_HIP( hipStreamSynchronize( s ) );
    return buildKdTreeDevice( ctx, sd.pts.p, cnt, sd.tree );
  };
  TMC2_TRY( upload( S, srcXyz, n ) );
  TMC2_TRY( upload( T, tgtXyz, m ) );
  std::vector<uint8_t> c4( 4 * n );
  for ( uint64_t i = 0; i < n; ++i ) c4[4 * i] = srcRgb[3 * i], c4[4 * i + 1] = srcRgb[3 * i + 1], c4[4 * i + 2] = srcRgb[3 * i + 2], c4[4 * i + 3] = 0;
  DevBuf<uint8_t>  d_rgb, d_out;
  DevBuf<uint32_t> d_err;
  TMC2_TRY( d_rgb.alloc( 4 * n ) );
  TMC2_TRY( d_out.alloc( 4 * m ) );
  TMC2_TRY( d_err.alloc( 1 ) );
  TMC2_HIP( hipMemcpyAsync( d_rgb.p, c4.data(), 4 * n, hipMemcpyHostToDevice, s ) );
  TMC2_TRY( transferColorsDevice( ctx, S.tree.view( QueryBox::Any ), S.pts.p, d_rgb.p, uint32_t( n ), T.tree.view( QueryBox::Any ), T.pts.p,
                                  uint32_t( m ), d_out.p, d_err.p, params ) );
  std::vector<uint8_t> o4( 4 * m );
  uint32_t             err = 0;
  TMC2_HIP( hipMemcpyAsync( o4.data(), d_out.p, 4 * m, hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipMemcpyAsync( &err, d_err.p, 4, hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipStreamSynchronize( s ) );
  if ( err ) {
    setError( "transferColors: a backward candidate list hit std::sort's depth limit (not reproduced)" );
    return TMC2_E_UNSUPPORTED;
  }
  for ( uint64_t i = 0; i < m; ++i ) tgtRgb[3 * i] = o4[4 * i], tgtRgb[3 * i + 1] = o4[4 * i + 1], tgtRgb[3 * i + 2] = o4[4 * i + 2];
  return TMC2_OK;
}

// ... at the CTC point
int tmc2_transfer_colors( tmc2_ctx* ctx, const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n, const int16_t* tgtXyz,
                          uint64_t m, uint8_t* tgtRgb ) {
  if ( !ctx || !srcXyz || !srcRgb || !tgtXyz || !tgtRgb || n < 8 || m < 1 ) {
    tmc2::setError( "transfer_colors: invalid argument (the source needs at least 8 points)" );
    return TMC2_E_INVALID;
  }
  tmc2_color_transfer_params ctc;
  tmc2::ctDefault( ctc );
  return tmc2_transfer_colors_ex( ctx, srcXyz, srcRgb, n, tgtXyz, m, &ctc, tgtRgb );
}

int tmc2_codec_generate_point_cloud( tmc2_frame* f ) {
  if ( !f ) return TMC2_E_INVALID;
  tmc2::ApiScope scope( f->ctx );
  return tmc2::reconstructPointCloud( f );
}

int tmc2_encoder_generate_attribute_images_ex( tmc2_frame* f, const tmc2_color_transfer_params* params ) {
  if ( !f ) return TMC2_E_INVALID;
  if ( !params ) {
    tmc2::setError( "generateAttributeImages: the colour-transfer parameters are NULL" );
    return TMC2_E_INVALID;
  }
  tmc2::ApiScope scope( f->ctx );
  return tmc2::generateAttributeImages( f, params );
}

int tmc2_encoder_generate_attribute_images( tmc2_frame* f ) {
  if ( !f ) return TMC2_E_INVALID;
  tmc2_color_transfer_params ctc;
  tmc2::ctDefault( ctc );
  return tmc2_encoder_generate_attribute_images_ex( f, &ctc );
}

int64_t tmc2_frame_recon_count( tmc2_frame* f ) { return ( f && f->haveReconstruction ) ? int64_t( f->reconCount ) : 0; }

int tmc2_frame_get_reconstruction( tmc2_frame* f, int16_t* xyz, uint8_t* rgb, uint32_t* pointToPixel ) {
  if ( !f || !f->haveReconstruction ) {
    tmc2::setError( "get_reconstruction: not generated" );
    return TMC2_E_STATE;
  }
  if ( rgb && ( !f->haveAttributeImages || f->havePbf ) ) {  // (the colours are those of the plain reconstruction's points)
    tmc2::setError( "get_reconstruction: no transferred colours (tmc2_encoder_generate_attribute_images produces them)" );
    return TMC2_E_STATE;
  }
  tmc2::ApiScope scope( f->ctx );
  hipStream_t    s = f->ctx->stream;
  const size_t   M = f->reconCount;
  if ( M == 0 ) return TMC2_OK;  // (occupancy synthesis removed every pixel: nothing to copy)
  std::vector<tmc2::Pt>  pts( M );
  std::vector<uint8_t>   c4( rgb ? 4 * M : 0 );
  std::vector<uint32_t>  pp( M );
  TMC2_HIP( hipMemcpyAsync( pts.data(), f->d_recon.p, M * sizeof( tmc2::Pt ), hipMemcpyDeviceToHost, s ) );
  if ( rgb ) TMC2_HIP( hipMemcpyAsync( c4.data(), f->d_reconRgb.p, 4 * M, hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipMemcpyAsync( pp.data(), f->d_pointToPixel.p, 4 * M, hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipStreamSynchronize( s ) );
  for ( size_t i = 0; i < M; ++i ) {
    if ( xyz ) xyz[3 * i] = pts[i].x, xyz[3 * i + 1] = pts[i].y, xyz[3 * i + 2] = pts[i].z;
    if ( rgb ) rgb[3 * i] = c4[4 * i], rgb[3 * i + 1] = c4[4 * i + 1], rgb[3 * i + 2] = c4[4 * i + 2];
    if ( pointToPixel )
      pointToPixel[3 * i] = tmc2::pixelX( pp[i] ), pointToPixel[3 * i + 1] = tmc2::pixelY( pp[i] ), pointToPixel[3 * i + 2] = tmc2::pixelLayer( pp[i] );
  }
  return TMC2_OK;
}

int tmc2_frame_device_attribute( tmc2_frame* f, void** attribute ) {
  if ( !f || !attribute || !f->haveAttributeImages ) return TMC2_E_STATE;
  *attribute = f->d_attr.p;
  return TMC2_OK;
}

int tmc2_frame_get_attribute_images( tmc2_frame* f, uint8_t* attribute ) {
  if ( !f || !attribute || !f->haveAttributeImages ) {
    tmc2::setError( "get_attribute_images: not generated" );
    return TMC2_E_STATE;
  }
  tmc2::ApiScope scope( f->ctx );
  TMC2_HIP( hipMemcpyAsync( attribute, f->d_attr.p, size_t( 6 ) * f->canvasW * f->canvasH, hipMemcpyDeviceToHost, f->ctx->stream ) );
  TMC2_HIP( hipStreamSynchronize( f->ctx->stream ) );
  return TMC2_OK;
}
}
