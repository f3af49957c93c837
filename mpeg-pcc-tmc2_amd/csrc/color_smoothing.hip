// color_smoothing.hip -- T6 of the post-reconstruction tail on gfx950: attribute (colour) smoothing.
//
// Replaces (reference: source/lib/...)
//   T6  PCCCodec::colorSmoothing                     PccLibCommon/source/PCCCodec.cpp:151-238 with addGridColorCentroid :1170-1191,
//                                                    gridFilteringColor :1193-1277, smoothPointCloudColorLC :1279-1317 and
//                                                    mean / median of PCCCodec.h:270-283; the branch between transferColors16bitBP
//                                                    and convertYUV16ToRGB8 (PCCEncoder.cpp:701-705, PCCDecoder.cpp:463)
//
// The twin of T3 (post_reconstruct.hip) on colours, with three differences that shape the kernels:
//  * the grid spans the whole cube (2^geometryBitDepth3D / gridSize cells a side, gridSize = occupancyPrecision: 512^3 at 11
//    bits).  The marked cells are T3's form (markedCells, cell_grid.hip): one bit each plus a rank per 32-bit word.
//  * a cell needs the median of its lumas, so the points of every marked cell are brought together first (count, prefix sum,
//    scatter of the point indices -- the count is the only atomic) and ONE wavefront per cell makes every reduction of that
//    cell from its segment: count, the three colour sums, "a second patch showed up", mean against median.
//  * the reference adds a cell's colours in float, in point order.  Integer sums below 2^24 are exact in any order; a cell at
//    or above that (256 points and more) is added again in float in point-index order by the same wavefront.
// The filter of a point reads the cell table and its own colour only, so colours are rewritten in place.
#include <algorithm>

#include "cell_grid.h"
#include "color_smoothing.h"
#include "internal.h"
#include "wave.h"

namespace tmc2 {
namespace {

// where a point's patch comes from: an array (host-array entry) or the frame's canvases (as T3: blockToPatch through pointToPixel)
struct PatchSource {
  const uint32_t* patchIndex;
  const uint32_t* pointToPixel;
  const uint32_t* blockToPatch;
  int             Wb;
  __device__ __forceinline__ uint32_t of( uint32_t i ) const {
    if ( patchIndex ) return patchIndex[i];
    const uint32_t p = pointToPixel[i];
    return blockToPatch[size_t( pixelY( p ) / 16 ) * Wb + pixelX( p ) / 16];
  }
};

// error words: [0] a point outside the cube, [1] the largest count of a cell beyond kCellMaxCount
// every point (any boundary type) whose own cell is marked belongs to that cell
__global__ __launch_bounds__( 256 ) void countCellPointsKernel( const Pt* __restrict__ pts, uint32_t M, CellGrid g,
                                                                 const uint32_t* __restrict__ bits, const uint32_t* __restrict__ rank,
                                                                 uint32_t* __restrict__ pointSlot, uint32_t* __restrict__ cellCount,
                                                                 uint32_t* __restrict__ error ) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i >= M ) return;
  const Pt p    = pts[i];
  uint32_t slot = kNoSlot;
  if ( !csInCube( g, p.x, p.y, p.z ) ) {
    error[0] = 1u;
  } else {
    slot = slotOfKey( bits, rank, g.keyOfPoint( p.x, p.y, p.z ) );
    if ( slot != kNoSlot ) atomicAdd( &cellCount[slot], 1u );
  }
  pointSlot[i] = slot;
}

__global__ __launch_bounds__( 256 ) void scatterCellPointsKernel( const uint32_t* __restrict__ pointSlot, uint32_t M,
                                                                   const uint32_t* __restrict__ cellOffset, uint32_t* __restrict__ cursor,
                                                                   uint32_t* __restrict__ entries ) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i >= M ) return;
  const uint32_t slot = pointSlot[i];
  if ( slot != kNoSlot ) entries[cellOffset[slot] + atomicAdd( &cursor[slot], 1u )] = i;
}

// The value of rank k (0-based, sorted ascending) among the lumas of a segment of more than 64 points: two passes of a
// 256-bin histogram in LDS (high byte, then low byte among the values of that high byte).  One wavefront = one workgroup.
__device__ uint32_t selectLuma( const uint32_t* __restrict__ seg, uint32_t n, const ushort4* __restrict__ colors, uint32_t k,
                                uint32_t* hist, int lane ) {
  uint32_t prefix = 0;  // the high byte, once known
  for ( int pass = 0; pass < 2; ++pass ) {
    __syncthreads();
    for ( int b = lane; b < 256; b += 64 ) hist[b] = 0;
    __syncthreads();
    for ( uint32_t e = lane; e < n; e += 64 ) {
      const uint32_t v = colors[seg[e]].x;
      if ( pass == 0 )
        atomicAdd( &hist[v >> 8], 1u );
      else if ( ( v >> 8 ) == prefix )
        atomicAdd( &hist[v & 255u], 1u );
    }
    __syncthreads();
    // lane l owns bins 4l .. 4l+3: the bin in which the running count passes k
    const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
    const uint32_t inc = waveInclusive( h0 + h1 + h2 + h3, lane );
    const unsigned long long past  = __ballot( inc > k );
    const int                owner = __ffsll( static_cast<long long>( past ) ) - 1;  // (k < n: some lane passes it)
    uint32_t                 bin = 0, before = 0;
    if ( lane == owner ) {
      before = inc - ( h0 + h1 + h2 + h3 );
      bin    = 4 * lane;
      if ( before + h0 <= k ) {
        before += h0, ++bin;
        if ( before + h1 <= k ) {
          before += h1, ++bin;
          if ( before + h2 <= k ) before += h2, ++bin;
        }
      }
    }
    bin    = __shfl( bin, owner, 64 );
    before = __shfl( before, owner, 64 );
    k -= before;
    if ( pass == 0 )
      prefix = bin;
    else
      prefix = ( prefix << 8 ) | bin;
  }
  return prefix;
}

// one wavefront (= one workgroup) per marked cell: every reduction of the cell from its segment of point indices
__global__ __launch_bounds__( 64 ) void cellStatsKernel( const uint32_t* __restrict__ cellCount, const uint32_t* __restrict__ cellOffset,
                                                          uint32_t cells, const uint32_t* __restrict__ entries,
                                                          const ushort4* __restrict__ colors, PatchSource patches,
                                                          double thresholdColorVariation, ColorCell* __restrict__ table,
                                                          uint32_t* __restrict__ error ) {
  __shared__ uint32_t hist[256];
  const int lane = threadIdx.x;
  for ( uint32_t cell = blockIdx.x; cell < cells; cell += gridDim.x ) {
    const uint32_t n = cellCount[cell];
    ColorCell      out{n, {0.f, 0.f, 0.f}, 0u};
    if ( n == 0 || n > kCellMaxCount ) {
      if ( lane == 0 ) {
        if ( n > kCellMaxCount ) atomicMax( &error[1], n );
        table[cell] = out;
      }
      continue;
    }
    const uint32_t* seg = entries + cellOffset[cell];
    uint32_t        s0 = 0, s1 = 0, s2 = 0, pMin = 0xFFFFFFFFu, pMax = 0u;  // (65535 points x 65535 fit 32 bits)
    uint32_t        mine = 0xFFFFFFFFu;                                     // n <= 64: the luma of entry `lane`
    for ( uint32_t e = lane; e < n; e += 64 ) {
      const uint32_t idx = seg[e];
      const ushort4  c   = colors[idx];
      const uint32_t p   = patches.of( idx );
      s0 += c.x, s1 += c.y, s2 += c.z;
      pMin = min( pMin, p ), pMax = max( pMax, p );
      mine = c.x;
    }
    s0 = waveSum( s0 ), s1 = waveSum( s1 ), s2 = waveSum( s2 );
    pMin = waveMin( pMin ), pMax = waveMax( pMax );
    uint32_t medianLo = 0, medianHi = 0;
    if ( n > 1 ) {
      if ( n <= 64 ) {  // rank of every value by counting, ties by lane
        uint32_t r = 0;
        for ( uint32_t j = 0; j < n; ++j ) {
          const uint32_t v = __shfl( mine, int( j ), 64 );
          r += ( v < mine || ( v == mine && int( j ) < lane ) ) ? 1u : 0u;
        }
        const bool               live = uint32_t( lane ) < n;
        const unsigned long long hi   = __ballot( live && r == n / 2 ), lo = __ballot( live && r + 1 == n / 2 );
        medianHi                      = __shfl( mine, __ffsll( static_cast<long long>( hi ) ) - 1, 64 );
        medianLo                      = lo ? uint32_t( __shfl( mine, __ffsll( static_cast<long long>( lo ) ) - 1, 64 ) ) : 0u;
      } else {
        medianHi = selectLuma( seg, n, colors, n / 2, hist, lane );
        medianLo = ( n % 2 == 0 ) ? selectLuma( seg, n, colors, n / 2 - 1, hist, lane ) : 0u;
      }
    }
    out.flags = csCellFlags( n, s0, medianLo, medianHi, pMin != pMax, thresholdColorVariation );
    if ( s0 < kCellExactSum && s1 < kCellExactSum && s2 < kCellExactSum ) {
      out.sum[0] = float( s0 ), out.sum[1] = float( s1 ), out.sum[2] = float( s2 );
    } else {
      // the reference's float additions in point order: the next smallest index of the segment, n times over
      float    f0 = 0.f, f1 = 0.f, f2 = 0.f;
      uint32_t prev = 0;
      for ( uint32_t t = 0; t < n; ++t ) {
        uint32_t next = 0xFFFFFFFFu;
        for ( uint32_t e = lane; e < n; e += 64 ) {
          const uint32_t idx = seg[e];
          if ( ( t == 0 || idx > prev ) && idx < next ) next = idx;
        }
        next            = waveMin( next );
        const ushort4 c = colors[next];
        f0 = __fadd_rn( f0, float( c.x ) ), f1 = __fadd_rn( f1, float( c.y ) ), f2 = __fadd_rn( f2, float( c.z ) );
        prev = next;
      }
      out.sum[0] = f0, out.sum[1] = f1, out.sum[2] = f2;
    }
    if ( lane == 0 ) table[cell] = out;
  }
}

struct CellLookup {
  CellGrid         g;
  const uint32_t*  bits;
  const uint32_t*  rank;
  const ColorCell* table;
  __device__ __forceinline__ ColorCell operator()( int cx, int cy, int cz ) const {
    const uint32_t slot = slotOfKey( bits, rank, g.key( cx, cy, cz ) );
    return slot == kNoSlot ? ColorCell{0u, {0.f, 0.f, 0.f}, 0u} : table[slot];
  }
};

__global__ __launch_bounds__( 256 ) void filterColorsKernel( const Pt* __restrict__ pts, const uint8_t* __restrict__ btype, uint32_t M,
                                                              CellLookup cells, double thresholdSmoothing, double thresholdDifference,
                                                              ushort4* __restrict__ colors ) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i >= M || btype[i] != 1 ) return;
  const Pt p = pts[i];
  if ( cells.g.outside( p.x, p.y, p.z ) ) return;
  const int      P[3]   = {p.x, p.y, p.z};
  const ushort4  c      = colors[i];
  const uint16_t own[3] = {c.x, c.y, c.z};
  uint16_t       res[3];
  if ( csFilterPoint( cells.g, P, own, cells, thresholdSmoothing, thresholdDifference, res ) )
    colors[i] = make_ushort4( res[0], res[1], res[2], 0 );
}

int checkParameters( const char* who, int gridSize, int bits3d ) {
  if ( !colorGridSupported( gridSize, bits3d ) ) {
    setError( "%s: gridSize %d at geometryBitDepth3D %d unsupported (grid sizes 2, 4, 8, 16; at most 2^31 cells)", who, gridSize, bits3d );
    return TMC2_E_UNSUPPORTED;
  }
  return TMC2_OK;
}
}  // namespace

// d_pts / d_btype / d_colors: M points on the device; colours are rewritten in place
int colorSmoothingDevice( tmc2_ctx* ctx, const Pt* d_pts, const uint8_t* d_btype, uint64_t* d_colors, uint32_t M,
                          const uint32_t* d_patchIndex, const uint32_t* d_pointToPixel, const uint32_t* d_blockToPatch, int Wb, int gridSize,
                          int bits3d, double thrSmoothing, double thrDifference, double thrVariation ) {
  TMC2_TRY( checkParameters( "colorSmoothing", gridSize, bits3d ) );
  if ( M == 0 ) return TMC2_OK;
  hipStream_t    s = ctx->stream;
  const CellGrid g = cubeCellGrid( gridSize, bits3d );
  const dim3     blk( 256 ), grdM( ( M + 255 ) / 256 );
  MarkedCells      marked;
  DevBuf<uint32_t> d_small, d_pointSlot, d_entries;
  TMC2_TRY( d_small.alloc( 4 ) );
  TMC2_TRY( d_pointSlot.alloc( M ) );
  TMC2_TRY( d_entries.alloc( M ) );
  StageScope stage( ctx, "color_smoothing" );
  TMC2_HIP( hipMemsetAsync( d_small.p, 0, 16, s ) );
  TMC2_TRY( markedCells( ctx, d_pts, d_btype, M, g, d_small.p, marked ) );
  const uint32_t cells = marked.count;
  if ( cells == 0 ) return TMC2_OK;  // no boundary point inside the faces: nothing is filtered
  DevBuf<uint32_t>  d_count, d_offset, d_cursor;
  DevBuf<ColorCell> d_table;
  TMC2_TRY( d_count.alloc( cells ) );
  TMC2_TRY( d_offset.alloc( cells ) );
  TMC2_TRY( d_cursor.alloc( cells ) );
  TMC2_TRY( d_table.alloc( cells ) );
  TMC2_HIP( hipMemsetAsync( d_count.p, 0, size_t( cells ) * 4, s ) );
  TMC2_HIP( hipMemsetAsync( d_cursor.p, 0, size_t( cells ) * 4, s ) );
  hipLaunchKernelGGL( countCellPointsKernel, grdM, blk, 0, s, d_pts, M, g, marked.bits.p, marked.rank.p, d_pointSlot.p, d_count.p, d_small.p + 1 );
  TMC2_TRY( exclusiveScanU32( ctx, d_count.p, d_offset.p, cells, nullptr ) );
  hipLaunchKernelGGL( scatterCellPointsKernel, grdM, blk, 0, s, d_pointSlot.p, M, d_offset.p, d_cursor.p, d_entries.p );
  const PatchSource patches{d_patchIndex, d_pointToPixel, d_blockToPatch, Wb};
  ushort4*          colors = reinterpret_cast<ushort4*>( d_colors );
  hipLaunchKernelGGL( cellStatsKernel, dim3( uint32_t( std::min<size_t>( cells, size_t( 32 ) * ctx->cuCount ) ) ), dim3( 64 ), 0, s, d_count.p,
                      d_offset.p, cells, d_entries.p, colors, patches, thrVariation, d_table.p, d_small.p + 1 );
  const CellLookup lookup{g, marked.bits.p, marked.rank.p, d_table.p};
  hipLaunchKernelGGL( filterColorsKernel, grdM, blk, 0, s, d_pts, d_btype, M, lookup, thrSmoothing, thrDifference, colors );
  stage.end();
  uint32_t err[2] = {0, 0};
  TMC2_HIP( hipMemcpyAsync( err, d_small.p + 1, 8, hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipStreamSynchronize( s ) );
  TMC2_HIP( hipGetLastError() );
  if ( err[0] ) {
    setError( "colorSmoothing: a point lies outside the cube of %d^3 (geometryBitDepth3D %d)", g.th, bits3d );
    return TMC2_E_INVALID;
  }
  if ( err[1] ) {
    setError( "colorSmoothing: a grid cell holds %u points, more than 65535 (the reference's uint16 count wraps there)", err[1] );
    return TMC2_E_UNSUPPORTED;
  }
  return TMC2_OK;
}

int colorSmoothingFrame( tmc2_frame* f, int gridSize, double thrSmoothing, double thrDifference, double thrVariation ) {
  if ( !f->haveReconstruction || f->reconCount == 0 || !f->haveColors16 || !f->haveBoundaryTypes ) {
    setError( "colorSmoothing: needs the finished cloud's 16-bit colours and boundary types (tmc2_codec_color_point_cloud, "
              "tmc2_codec_smooth_point_cloud_postprocess, tmc2_codec_transfer_colors_16bit_bp first)" );
    return TMC2_E_STATE;
  }
  if ( f->geometryBitDepth3D == 0 ) {
    setError( "colorSmoothing: the frame's geometryBitDepth3D is unknown (tmc2_segmenter_compute sets it; "
              "tmc2_frame_set_geometry_bit_depth_3d for a decoder-side frame)" );
    return TMC2_E_STATE;
  }
  const Pt* pts = f->haveSmoothed ? f->d_reconSmoothed.p : f->d_recon.p;
  TMC2_TRY( colorSmoothingDevice( f->ctx, pts, f->d_boundaryType.p, f->d_colors16.p, uint32_t( f->reconCount ), nullptr, f->d_pointToPixel.p,
                                  f->d_blockToPatch.p, f->canvasW / 16, gridSize, f->geometryBitDepth3D, thrSmoothing, thrDifference,
                                  thrVariation ) );
  f->haveRgbPost = false;
  return TMC2_OK;
}

}  // namespace tmc2

extern "C" {

int tmc2_frame_set_geometry_bit_depth_3d( tmc2_frame* f, int geometryBitDepth3D ) {
  if ( !f || geometryBitDepth3D < 1 || geometryBitDepth3D > 14 ) {
    tmc2::setError( "set_geometry_bit_depth_3d: invalid argument" );
    return TMC2_E_INVALID;
  }
  f->geometryBitDepth3D = geometryBitDepth3D;
  return TMC2_OK;
}

int tmc2_codec_color_smoothing( tmc2_frame* f, int gridSize, double thresholdColorSmoothing, double thresholdColorDifference,
                                double thresholdColorVariation ) {
  if ( !f ) return TMC2_E_INVALID;
  tmc2::ApiScope scope( f->ctx );
  return tmc2::colorSmoothingFrame( f, gridSize, thresholdColorSmoothing, thresholdColorDifference, thresholdColorVariation );
}

int tmc2_color_smoothing( tmc2_ctx* ctx, const int16_t* xyz, uint16_t* colors16, const uint16_t* boundaryType, const uint32_t* patchIndex,
                          uint64_t M, int gridSize, int geometryBitDepth3D, double thresholdColorSmoothing, double thresholdColorDifference,
                          double thresholdColorVariation ) {
  using namespace tmc2;
  if ( !ctx || ( M && ( !xyz || !colors16 || !boundaryType || !patchIndex ) ) || M > 0xFFFFFFF0ull ) {
    setError( "color_smoothing: invalid argument" );
    return TMC2_E_INVALID;
  }
  ApiScope scope( ctx );
  TMC2_TRY( checkParameters( "color_smoothing", gridSize, geometryBitDepth3D ) );
  if ( M == 0 ) return TMC2_OK;
  hipStream_t           s = ctx->stream;
  std::vector<Pt>       pts( M );
  std::vector<uint64_t> c4( M );
  std::vector<uint8_t>  bt( M );
  for ( uint64_t i = 0; i < M; ++i ) {
    pts[i] = Pt{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0};
    c4[i]  = uint64_t( colors16[3 * i] ) | ( uint64_t( colors16[3 * i + 1] ) << 16 ) | ( uint64_t( colors16[3 * i + 2] ) << 32 );
    bt[i]  = uint8_t( std::min<uint16_t>( boundaryType[i], 255 ) );
  }
  DevBuf<Pt>       d_pts;
  DevBuf<uint64_t> d_colors;
  DevBuf<uint8_t>  d_bt;
  DevBuf<uint32_t> d_patch;
  TMC2_TRY( d_pts.alloc( M ) );
  TMC2_TRY( d_colors.alloc( M ) );
  TMC2_TRY( d_bt.alloc( M ) );
  TMC2_TRY( d_patch.alloc( M ) );
  TMC2_HIP( hipMemcpyAsync( d_pts.p, pts.data(), M * sizeof( Pt ), hipMemcpyHostToDevice, s ) );
  TMC2_HIP( hipMemcpyAsync( d_colors.p, c4.data(), M * 8, hipMemcpyHostToDevice, s ) );
  TMC2_HIP( hipMemcpyAsync( d_bt.p, bt.data(), M, hipMemcpyHostToDevice, s ) );
  TMC2_HIP( hipMemcpyAsync( d_patch.p, patchIndex, M * 4, hipMemcpyHostToDevice, s ) );
  TMC2_HIP( hipStreamSynchronize( s ) );  // the caller's and the staging buffers are free again
  TMC2_TRY( colorSmoothingDevice( ctx, d_pts.p, d_bt.p, d_colors.p, uint32_t( M ), d_patch.p, nullptr, nullptr, 0, gridSize, geometryBitDepth3D,
                                  thresholdColorSmoothing, thresholdColorDifference, thresholdColorVariation ) );
  TMC2_HIP( hipMemcpyAsync( c4.data(), d_colors.p, M * 8, hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipStreamSynchronize( s ) );
  for ( uint64_t i = 0; i < M; ++i )
    for ( int k = 0; k < 3; ++k ) colors16[3 * i + k] = uint16_t( c4[i] >> ( 16 * k ) );
  return TMC2_OK;
}
}
