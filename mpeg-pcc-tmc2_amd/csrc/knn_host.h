// knn_host.h -- nanoflann's k-NN search restated on the host over tmc2_host_kdtree_build's tree: searchLevel as a recursion, its
// KNNResultSet::addPoint as a sorted array (insert behind equal distances, drop what equals the worst of a full list).  What the host
// restatements of the k-NN refinement (refine_knn_host.cpp) and of the colour transfer (color_transfer_host.cpp) search with.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <thread>
#include <vector>

#include "internal.h"

namespace tmc2 {

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
  // the whole search around ( x, y, z ): dist / pos [K] = squared distances and TREE positions in the reference's result order
  static void around( const KdTreeHost& t, int x, int y, int z, uint32_t K, uint32_t* dist, uint32_t* pos ) {
    HostSearch s{t, {x, y, z}, K, 0, dist, pos};
    int        o[3];  // (nanoflann computeInitialDistances: the offset of the query to the root box)
    for ( int d = 0; d < 3; ++d ) o[d] = s.q[d] < t.lo[d] ? t.lo[d] - s.q[d] : ( s.q[d] > t.hi[d] ? s.q[d] - t.hi[d] : 0 );
    s.level( 0, o );
  }
};

// the worker threads of a host entry: the machine's, at most 16 (rows and points are independent of each other)
inline unsigned hostWorkers( uint64_t items ) {
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

}  // namespace tmc2
