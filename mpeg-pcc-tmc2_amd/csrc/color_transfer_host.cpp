// color_transfer_host.cpp -- PCCPointSet3::transferColors (PccLibCommon/source/PCCPointSet.cpp:807-1124) restated on the host, with
// no device, over its sixteen arguments: nanoflann's searches over tmc2_host_kdtree_build's trees (knn_host.h), the backward lists
// appended in source order then result order and ordered by the replay of libstdc++'s std::sort (cand_sort.h), and the per-target
// rules of color_transfer_rules.h -- the text the device kernels run.  What the CPU test tier checks against the recorded
// reference results, and what the GPU tier holds the kernels against.  Also the parameter entries, which need no device either.
#include <vector>

#include "cand_sort.h"
#include "color_transfer_rules.h"
#include "internal.h"
#include "knn_host.h"

namespace tmc2 {

// TMC2_E_INVALID for a NULL set, TMC2_E_UNSUPPORTED with the field named; n / m: the clouds, 0 where they are not known yet
int checkColorTransferParams( const char* who, const tmc2_color_transfer_params* q, uint64_t n, uint64_t m ) {
  if ( !q ) {
    setError( "%s: the colour-transfer parameters are NULL", who );
    return TMC2_E_INVALID;
  }
  if ( const char* what = ctRefusal( *q ) ) {
    setError( "%s: unsupported %s", who, what );
    return TMC2_E_UNSUPPORTED;
  }
  if ( n > kCtMaxSource && !ctIsDefault( *q ) ) {  // (a backward entry is numbered source * K + rank in 32 bits, K <= 32; the CTC point's: source)
    setError( "%s: unsupported source of %llu points (the colour transfer numbers its backward entries in 32 bits: at most %llu)", who,
              (unsigned long long)n, (unsigned long long)kCtMaxSource );
    return TMC2_E_UNSUPPORTED;
  }
  if ( n && uint64_t( q->numNeighborsColorTransferFwd ) > n ) {
    setError( "%s: unsupported numNeighborsColorTransferFwd %d above the source's %llu points", who, q->numNeighborsColorTransferFwd,
              (unsigned long long)n );
    return TMC2_E_UNSUPPORTED;
  }
  if ( m && uint64_t( q->numNeighborsColorTransferBwd ) > m ) {
    setError( "%s: unsupported numNeighborsColorTransferBwd %d above the target's %llu points", who, q->numNeighborsColorTransferBwd,
              (unsigned long long)m );
    return TMC2_E_UNSUPPORTED;
  }
  return TMC2_OK;
}

namespace {
struct Entry {
  uint32_t x, y;  // squared distance, source
};
}  // namespace

}  // namespace tmc2

extern "C" {

void tmc2_color_transfer_params_default( tmc2_color_transfer_params* params ) {
  if ( params ) tmc2::ctDefault( *params );
}

int tmc2_color_transfer_params_check( const tmc2_color_transfer_params* params ) {
  return tmc2::checkColorTransferParams( "color_transfer_params_check", params, 0, 0 );
}

int tmc2_host_transfer_colors( const int16_t* srcXyz, const uint8_t* srcRgb, uint64_t n, const int16_t* tgtXyz, uint64_t m,
                               const tmc2_color_transfer_params* params, uint8_t* tgtRgb ) {
  using namespace tmc2;
  if ( !srcXyz || !srcRgb || !tgtXyz || !tgtRgb || n < 1 || m < 1 || n > 0x3FFFFFFull || m > 0x7FFFFFF0ull ) {
    setError( "host_transfer_colors: invalid argument" );
    return TMC2_E_INVALID;
  }
  TMC2_TRY( checkColorTransferParams( "host_transfer_colors", params, n, m ) );
  const CtRules p = ctRules( *params );
  KdTreeHost    S, T;
  S.build( srcXyz, n );
  T.build( tgtXyz, m );
  const auto srcColor = [&]( uint64_t i ) { return CtColor{srcRgb[3 * i], srcRgb[3 * i + 1], srcRgb[3 * i + 2]}; };
  // ---- forward
  std::vector<CtColor> fwd( m );
  const uint32_t       kf = uint32_t( p.kFwd ), kb = uint32_t( p.kBwd );
  parallelRanges( m, [&]( uint64_t from, uint64_t to ) {
    std::vector<uint32_t> dist( kf ), pos( kf );
    for ( uint64_t t = from; t < to; ++t ) {
      HostSearch::around( S, tgtXyz[3 * t], tgtXyz[3 * t + 1], tgtXyz[3 * t + 2], kf, dist.data(), pos.data() );
      fwd[t] = ctForward( p, int( kf ), [&]( int i ) { return dist[size_t( i )]; }, [&]( int i ) { return srcColor( S.perm[pos[size_t( i )]] ); } );
    }
  } );
  // ---- backward: every source point's results, then the lists in the order the reference appends them
  std::vector<uint32_t> bd( n * kb ), bt( n * kb );
  parallelRanges( n, [&]( uint64_t from, uint64_t to ) {
    std::vector<uint32_t> pos( kb );
    for ( uint64_t s = from; s < to; ++s ) {
      HostSearch::around( T, srcXyz[3 * s], srcXyz[3 * s + 1], srcXyz[3 * s + 2], kb, &bd[s * kb], pos.data() );
      for ( uint32_t r = 0; r < kb; ++r ) bt[s * kb + r] = T.perm[pos[r]];
    }
  } );
  std::vector<uint64_t> offset( m + 1, 0 );
  for ( uint64_t e = 0; e < n * kb; ++e )
    if ( double( bd[e] ) <= p.geoBwd ) ++offset[bt[e] + 1];
  for ( uint64_t t = 0; t < m; ++t ) offset[t + 1] += offset[t];
  std::vector<Entry>    entries( offset[m] );
  std::vector<uint64_t> cursor( offset.begin(), offset.end() - 1 );
  for ( uint64_t e = 0; e < n * kb; ++e )
    if ( double( bd[e] ) <= p.geoBwd ) entries[cursor[bt[e]]++] = Entry{bd[e], uint32_t( e / kb )};
  const double rTarget = 1.0 / double( m ), rSource = 1.0 / double( n );
  bool         sorted  = true;
  for ( uint64_t t = 0; t < m; ++t ) {
    const int cnt = int( offset[t + 1] - offset[t] );
    CtColor   c   = fwd[t];
    if ( cnt > 0 && !p.lossless ) {
      Entry* e = entries.data() + offset[t];
      sorted   = CandSortOf<Entry>{e}.sort( cnt ) && sorted;
      c = ctBackward( p, cnt, [&]( int i ) { return e[i].x; }, [&]( int i ) { return srcColor( e[i].y ); }, fwd[t], rTarget, rSource );
    }
    tgtRgb[3 * t] = uint8_t( c.c0 ), tgtRgb[3 * t + 1] = uint8_t( c.c1 ), tgtRgb[3 * t + 2] = uint8_t( c.c2 );
  }
  if ( !sorted ) {
    setError( "transferColors: a backward candidate list hit std::sort's depth limit (heapsort fallback of libstdc++ introsort is not reproduced)" );
    return TMC2_E_UNSUPPORTED;
  }
  return TMC2_OK;
}
}
