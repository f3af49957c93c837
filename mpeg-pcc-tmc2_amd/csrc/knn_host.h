// knn_host.h -- nanoflann's k-NN search restated on the host over tmc2_host_kdtree_build's tree: searchLevel as a recursion over the
// kernels' walk step (kd_walk.h), its KNNResultSet::addPoint as a sorted array (insert behind equal distances, drop what equals the
// worst of a full list).  What the host restatements of the k-NN refinement (refine_knn_host.cpp) and of the colour transfer
// (color_transfer_host.cpp) search with.
#pragma once
#include <algorithm>
#include <thread>
#include <vector>

#include "internal.h"
#include "kd_walk.h"

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
  void level( uint32_t node, const KdOffsets o ) {
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
    const KdStep st = kdStep( nd, q[0], q[1], q[2], o );
    level( st.nearC, o );
    if ( st.farMin <= worst() ) level( st.farC, st.far );
  }
  // the whole search around ( x, y, z ): dist / pos [K] = squared distances and TREE positions in the reference's result order
  static void around( const KdTreeHost& t, int x, int y, int z, uint32_t K, uint32_t* dist, uint32_t* pos ) {
    HostSearch s{t, {x, y, z}, K, 0, dist, pos};
    s.level( 0, kdInitialOffsets( kdBoxOf( t.lo, t.hi ), x, y, z ) );
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
