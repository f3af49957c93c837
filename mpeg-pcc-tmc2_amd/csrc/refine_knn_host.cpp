// refine_knn_host.cpp -- PCCPatchSegmenter3::refineSegmentation (PccLibEncoder/source/PCCPatchSegmenter.cpp:1322-1384) and the
// search behind its computeAdjacencyInfo (:267-291) restated on the host, with no device: nanoflann's searchLevel as a recursion
// over tmc2_host_kdtree_build's tree, its KNNResultSet::addPoint as a sorted array (insert behind equal distances, drop what
// equals the worst of a full list), then the Jacobi rounds with the vote of refine_knn.h -- the same text the device kernel runs.
// What the CPU test tier checks against the recorded reference results, and what the GPU tier holds the kernels against.
#include <thread>
#include <vector>

#include "internal.h"
#include "refine_knn.h"

namespace tmc2 {
namespace {

struct HostSearch {
  const KdTreeHost& t;
  int               q[3];
  uint32_t          K, count = 0;
  uint32_t *        dist, *pos;  // [K], sorted by (distance, order of arrival)
  uint32_t          worst() const { return count == K ? dist[K - 1] : 0xFFFFFFFFu; }
  void              add( uint32_t d, uint32_t p ) {
    uint32_t i = count;
    for ( ; i > 0 && dist[i - 1] > d; --i )
      if ( i < K ) dist[i] = dist[i - 1], pos[i] = pos[i - 1];
    if ( i < K ) dist[i] = d, pos[i] = p;
    if ( count < K ) ++count;
  }
  void level( uint32_t node, int o[3] ) {
    const KdNode& nd = t.nodes[node];
    if ( nd.dim < 0 ) {
      for ( int p = nd.a; p < nd.b; ++p ) {
        const Pt&      c  = t.ptsTree[size_t( p )];
        const int      ex = q[0] - c.x, ey = q[1] - c.y, ez = q[2] - c.z;
        const uint32_t d  = uint32_t( ex * ex + ey * ey + ez * ez );
        if ( d < worst() ) add( d, uint32_t( p ) );
      }
      return;
    }
    const int  v = q[nd.dim], diff1 = v - nd.divlow, diff2 = v - nd.divhigh;
    const bool leftNear = ( diff1 + diff2 ) < 0;
    level( leftNear ? uint32_t( nd.a ) : uint32_t( nd.b ), o );
    const int      kept = o[nd.dim], ofar = leftNear ? std::abs( diff2 ) : std::abs( diff1 );
    o[nd.dim]           = ofar;
    const uint32_t farMin = uint32_t( o[0] * o[0] + o[1] * o[1] + o[2] * o[2] );
    if ( farMin <= worst() ) level( leftNear ? uint32_t( nd.b ) : uint32_t( nd.a ), o );
    o[nd.dim] = kept;
  }
};

// the worker threads of the host entry: the machine's, at most 16 (rows and points are independent of each other)
unsigned hostWorkers( uint64_t items ) {
  const unsigned hw = std::max( 1u, std::thread::hardware_concurrency() );
  return unsigned( std::max<uint64_t>( 1, std::min<uint64_t>( std::min( hw, 16u ), items / 256 ) ) );
}
template <typename F>
void parallelRanges( uint64_t n, F body ) {
  const unsigned           workers = hostWorkers( n );
  std::vector<std::thread> pool;
  for ( unsigned w = 1; w < workers; ++w ) pool.emplace_back( body, n * w / workers, n * ( w + 1 ) / workers );
  body( uint64_t( 0 ), n / workers );
  for ( auto& th : pool ) th.join();
}

}  // namespace

// rows [n][K] of ORIGINAL indices, row i = the search around point i, in the order of the reference's result list
void knnWideHost( const KdTreeHost& t, uint32_t K, uint32_t* rows ) {
  std::vector<uint32_t> where( t.perm.size() );  // original index -> tree position
  for ( size_t p = 0; p < t.perm.size(); ++p ) where[t.perm[p]] = uint32_t( p );
  parallelRanges( t.perm.size(), [&]( uint64_t from, uint64_t to ) {
    std::vector<uint32_t> dist( K ), pos( K );
    for ( uint64_t i = from; i < to; ++i ) {
      HostSearch s{t, {0, 0, 0}, K, 0, dist.data(), pos.data()};
      const Pt& c = t.ptsTree[where[i]];
      s.q[0] = c.x, s.q[1] = c.y, s.q[2] = c.z;
      int o[3];  // (nanoflann computeInitialDistances: the offset of the query to the root box)
      for ( int d = 0; d < 3; ++d ) o[d] = s.q[d] < t.lo[d] ? t.lo[d] - s.q[d] : ( s.q[d] > t.hi[d] ? s.q[d] - t.hi[d] : 0 );
      s.level( 0, o );
      for ( uint32_t e = 0; e < K; ++e ) rows[i * K + e] = t.perm[pos[e]];
    }
  } );
}

// the rounds on rows [n][K]
void refineRoundsHost( const uint32_t* rows, uint64_t n, uint32_t K, const double* normals, uint32_t* partition, double lambda,
                       int iterationCount ) {
  const double         weight = lambda / double( K );
  std::vector<uint8_t> cur( n ), next( n );
  for ( uint64_t i = 0; i < n; ++i ) cur[i] = uint8_t( partition[i] );
  for ( int r = 0; r < iterationCount; ++r ) {
    std::atomic<bool> changed{false};
    parallelRanges( n, [&]( uint64_t from, uint64_t to ) {
      bool any = false;
      for ( uint64_t i = from; i < to; ++i ) {
        uint32_t count[6] = {0, 0, 0, 0, 0, 0};
        for ( uint32_t e = 0; e < K; ++e ) ++count[cur[rows[i * K + e]]];
        next[i] = uint8_t( refineVote( normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], cur[i], count, weight ) );
        any     = any || next[i] != cur[i];
      }
      if ( any ) changed.store( true );
    } );
    cur.swap( next );
    if ( !changed.load() ) break;  // a round is a function of the partition alone: a fixed point stays one
  }
  for ( uint64_t i = 0; i < n; ++i ) partition[i] = cur[i];
}

}  // namespace tmc2

extern "C" int tmc2_host_refine_segmentation( const int16_t* xyz, uint64_t n, const double* normals, uint32_t* partition, int maxNNCount,
                                              double lambda, int iterationCount, uint32_t* adjacency ) {
  using namespace tmc2;
  if ( !xyz || !normals || !partition || n == 0 || n > 0x7FFFFFF0ull ) {
    setError( "host_refine_segmentation: invalid argument" );
    return TMC2_E_INVALID;
  }
  int offending = 0;
  if ( const char* why = refineKnnRefusal( maxNNCount, lambda, iterationCount, &offending ) ) {
    char text[192];
    snprintf( text, sizeof( text ), why, offending );
    setError( "host_refine_segmentation: %s", text );
    return TMC2_E_UNSUPPORTED;
  }
  if ( uint64_t( maxNNCount ) > n ) {
    setError( "host_refine_segmentation: maxNNCountRefineSegmentation %d larger than the cloud (%llu points)", maxNNCount, (unsigned long long)n );
    return TMC2_E_UNSUPPORTED;
  }
  for ( uint64_t i = 0; i < n; ++i )
    if ( partition[i] > 5 ) {
      setError( "host_refine_segmentation: label %u of point %llu out of range (0..5)", partition[i], (unsigned long long)i );
      return TMC2_E_INVALID;
    }
  KdTreeHost t;
  t.build( xyz, n );
  std::vector<uint32_t> own;
  uint32_t*             rows = adjacency;
  if ( !rows ) {
    own.resize( n * size_t( maxNNCount ) );
    rows = own.data();
  }
  knnWideHost( t, uint32_t( maxNNCount ), rows );
  refineRoundsHost( rows, n, uint32_t( maxNNCount ), normals, partition, lambda, iterationCount );
  return TMC2_OK;
}
