// refine_knn_host.cpp -- PCCPatchSegmenter3::refineSegmentation (PccLibEncoder/source/PCCPatchSegmenter.cpp:1322-1384) and the
// search behind its computeAdjacencyInfo (:267-291) restated on the host, with no device: nanoflann's search over
// tmc2_host_kdtree_build's tree (knn_host.h), then the Jacobi rounds with the vote of refine_knn.h -- the same text the device kernel runs.
// What the CPU test tier checks against the recorded reference results, and what the GPU tier holds the kernels against.
#include <thread>
#include <vector>

#include "internal.h"
#include "knn_host.h"
#include "refine_knn.h"

namespace tmc2 {

// rows [n][K] of ORIGINAL indices, row i = the search around point i, in the order of the reference's result list
void knnWideHost( const KdTreeHost& t, uint32_t K, uint32_t* rows ) {
  std::vector<uint32_t> where( t.perm.size() );  // original index -> tree position
  for ( size_t p = 0; p < t.perm.size(); ++p ) where[t.perm[p]] = uint32_t( p );
  parallelRanges( t.perm.size(), [&]( uint64_t from, uint64_t to ) {
    std::vector<uint32_t> dist( K ), pos( K );
    for ( uint64_t i = from; i < to; ++i ) {
      const Pt& c = t.ptsTree[where[i]];
      HostSearch::around( t, c.x, c.y, c.z, K, dist.data(), pos.data() );
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
