// patch_border_filter_host.cpp -- PatchBlockFiltering::patchBorderFiltering (PccLibCommon/source/PCCPatch.cpp:797-976) restated
// on the host, with no device: the padded maps of every patch, its border points in raster order, the landings in the
// reference's order (neighbour patches ascending, their points in raster order, the first of the nearest stays), the passes
// and the border flags through the per-pixel text of patch_border_filter.h -- the same text the device kernels run.  What the
// CPU test tier checks against the recorded reference results, and what the GPU tier holds the kernels against on canvases no
// fixture covers.
#include <vector>

#include "internal.h"
#include "patch_border_filter.h"

namespace tmc2 {
namespace {
struct HostPatchMaps {
  int                  w = 0, h = 0;
  std::vector<uint8_t> occ;
  std::vector<int16_t> depth;
  struct BorderPoint {
    int16_t p[3];
  };
  std::vector<BorderPoint> points;
  PbfBox                   box;
};
}  // namespace

// what a canvas has to satisfy before anything indexes with it (shared with the frame entry)
int checkPbfPatch( const tmc2_patch& t, int k, int W, int H, const char* who ) {
  const int axes = ( 1 << ( t.normalAxis & 3 ) ) | ( 1 << ( t.tangentAxis & 3 ) ) | ( 1 << ( t.bitangentAxis & 3 ) );
  if ( t.normalAxis < 0 || t.normalAxis > 2 || t.tangentAxis < 0 || t.tangentAxis > 2 || t.bitangentAxis < 0 || t.bitangentAxis > 2 ||
       axes != 7 || t.projectionMode < 0 || t.projectionMode > 1 || t.sizeU0 <= 0 || t.sizeV0 <= 0 ) {
    setError( "%s: patch %d: axes (%d, %d, %d) / projection mode %d / block size %dx%d invalid", who, k, t.normalAxis, t.tangentAxis,
              t.bitangentAxis, t.projectionMode, t.sizeU0, t.sizeV0 );
    return TMC2_E_INVALID;
  }
  if ( t.patchOrientation != 0 && t.patchOrientation != 1 ) {
    setError( "%s: patch %d: patchOrientation %d unsupported (0 and 1 are)", who, k, t.patchOrientation );
    return TMC2_E_UNSUPPORTED;
  }
  const int64_t bw = t.patchOrientation == 0 ? t.sizeU0 : t.sizeV0, bh = t.patchOrientation == 0 ? t.sizeV0 : t.sizeU0;
  if ( t.u0 < 0 || t.v0 < 0 || ( int64_t( t.u0 ) + bw ) * 16 > W || ( int64_t( t.v0 ) + bh ) * 16 > H ) {
    setError( "%s: patch %d lies outside the %dx%d canvas", who, k, W, H );
    return TMC2_E_INVALID;
  }
  return TMC2_OK;
}

int patchBorderFilteringHost( const tmc2_patch* patches, int count, int W, int H, int prec, const uint8_t* occVideo, const uint16_t* geo0,
                              const uint32_t* blockToPatch, const PbfParams& q, uint8_t* occupancy, uint8_t* border ) {
  if ( W <= 0 || H <= 0 || W % 16 || H % 16 || W > kMaxCanvasDim || H > kMaxCanvasDim ) {
    setError( "host_patch_border_filtering: unsupported canvas %dx%d (multiples of 16, at most %d a side)", W, H, kMaxCanvasDim );
    return TMC2_E_UNSUPPORTED;
  }
  if ( const char* what = pbfRefusal( prec, q, count ) ) {
    setError( "host_patch_border_filtering: unsupported %s", what );
    return TMC2_E_UNSUPPORTED;
  }
  for ( int k = 0; k < count; ++k ) TMC2_TRY( checkPbfPatch( patches[k], k, W, H, "host_patch_border_filtering" ) );
  const int b = pbfBorder( prec ), Wv = W / prec, Wb = W / 16;
  std::vector<HostPatchMaps> maps( size_t( std::max( count, 0 ) ) );
  // ---- local maps, border points, boxes ---------------------------------------------------------------------------------
  for ( int k = 0; k < count; ++k ) {
    const tmc2_patch& t = patches[k];
    HostPatchMaps&    m = maps[size_t( k )];
    m.w = t.sizeU0 * 16 + 2 * b, m.h = t.sizeV0 * 16 + 2 * b;
    m.occ.assign( size_t( m.w ) * m.h, 0 );
    m.depth.assign( size_t( m.w ) * m.h, 0 );
    for ( int vb = 0; vb < t.sizeV0; ++vb )
      for ( int ub = 0; ub < t.sizeU0; ++ub ) {
        const int bx = t.patchOrientation == 0 ? ub + t.u0 : vb + t.u0, by = t.patchOrientation == 0 ? vb + t.v0 : ub + t.v0;
        if ( blockToPatch[size_t( by ) * Wb + bx] != uint32_t( k ) + 1u ) continue;
        for ( int v = vb * 16; v < vb * 16 + 16; ++v )
          for ( int u = ub * 16; u < ub * 16 + 16; ++u ) {
            const int x = t.patchOrientation == 0 ? u + t.u0 * 16 : v + t.u0 * 16, y = t.patchOrientation == 0 ? v + t.v0 * 16 : u + t.v0 * 16;
            if ( int( occVideo[size_t( y / prec ) * Wv + x / prec] ) <= q.thresholdLossyOM ) continue;
            const size_t c = size_t( v + b ) * m.w + u + b;
            m.occ[c]       = 1;
            m.depth[c]     = int16_t( geo0[size_t( y ) * W + x] );
          }
      }
    for ( int a = 0; a < 3; ++a ) m.box.lo[a] = 32767, m.box.hi[a] = -32768;
    for ( int v = 0; v < t.sizeV0 * 16; ++v )
      for ( int u = 0; u < t.sizeU0 * 16; ++u ) {
        const int64_t c = int64_t( v + b ) * m.w + u + b;
        if ( !pbfIsBorderPoint( m.occ.data(), c, m.w ) ) continue;
        HostPatchMaps::BorderPoint p;
        p.p[t.tangentAxis]   = int16_t( u + t.u1 );
        p.p[t.bitangentAxis] = int16_t( v + t.v1 );
        p.p[t.normalAxis]    = int16_t( pbfNormalCoord( t.projectionMode, t.d1, m.depth[size_t( c )] ) );
        m.points.push_back( p );
        for ( int a = 0; a < 3; ++a ) m.box.lo[a] = std::min( m.box.lo[a], p.p[a] ), m.box.hi[a] = std::max( m.box.hi[a], p.p[a] );
      }
  }
  // ---- per patch: landings, passes, flags -----------------------------------------------------------------------------------
  const int            reach = q.log2Threshold * q.log2Threshold;
  std::vector<int16_t> nd;
  std::vector<uint8_t> ping, pong;
  size_t               at = 0;
  for ( int k = 0; k < count; ++k ) {
    const tmc2_patch&    t = patches[k];
    const HostPatchMaps& m = maps[size_t( k )];
    nd.assign( m.occ.size(), int16_t( kPbfUndefined ) );
    for ( int j = 0; j < count; ++j ) {
      if ( j == k || !pbfBoxesMeet( m.box, maps[size_t( j )].box ) ) continue;
      for ( const auto& p : maps[size_t( j )].points ) {
        if ( !pbfInGrownBox( m.box, p.p ) ) continue;
        const int     d  = pbfDepthIn( t.projectionMode, t.d1, p.p[t.normalAxis] );
        const int64_t cu = int64_t( p.p[t.tangentAxis] ) - t.u1 + b, cv = int64_t( p.p[t.bitangentAxis] ) - t.v1 + b;
        if ( cu < 0 || cv < 0 || cu >= m.w || cv >= m.h ) continue;  // (only a coordinate that wrapped in its int16 gets here)
        const size_t c    = size_t( cv ) * m.w + size_t( cu );
        const int    dist = std::abs( d - int( m.depth[c] ) );
        if ( dist <= reach && dist < std::abs( int( nd[c] ) - int( m.depth[c] ) ) ) nd[c] = int16_t( d );
      }
    }
    ping = m.occ;
    pong.assign( m.occ.size(), 0 );
    for ( int pass = 0; pass < q.passesCount; ++pass ) {
      for ( int v = 0; v < t.sizeV0 * 16; ++v )
        for ( int u = 0; u < t.sizeU0 * 16; ++u ) {
          const int64_t c   = int64_t( v + b ) * m.w + u + b;
          pong[size_t( c )] = pbfKeepPixel( ping.data(), m.depth.data(), nd.data(), c, m.w, q.filterSize );
        }
      ping.swap( pong );
    }
    for ( int v = 0; v < t.sizeV0 * 16; ++v )
      for ( int u = 0; u < t.sizeU0 * 16; ++u, ++at ) {
        const int64_t c = int64_t( v + b ) * m.w + u + b;
        if ( occupancy ) occupancy[at] = ping[size_t( c )];
        if ( border ) border[at] = pbfBorderFlag( ping.data(), c, m.w );
      }
  }
  return TMC2_OK;
}
}  // namespace tmc2

extern "C" int tmc2_host_patch_border_filtering( const tmc2_patch* patches, int count, int width, int height, int occupancyPrecision,
                                                 const uint8_t* occVideo, const uint16_t* geometryD0, const uint32_t* blockToPatch,
                                                 int thresholdLossyOM, int passesCount, int filterSize, int log2Threshold,
                                                 uint8_t* occupancy, uint8_t* border ) {
  if ( count < 0 || ( count && !patches ) || !occVideo || !geometryD0 || !blockToPatch ) {
    tmc2::setError( "host_patch_border_filtering: invalid argument" );
    return TMC2_E_INVALID;
  }
  const tmc2::PbfParams q{thresholdLossyOM, passesCount, filterSize, log2Threshold};
  return tmc2::patchBorderFilteringHost( patches, count, width, height, occupancyPrecision, occVideo, geometryD0, blockToPatch, q, occupancy,
                                         border );
}
