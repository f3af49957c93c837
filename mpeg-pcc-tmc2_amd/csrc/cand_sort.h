// cand_sort.h -- libstdc++'s std::sort replayed, for the candidate lists of the colour transfers: on the device, and by the host
// restatement of the transfer (color_transfer_host.cpp) through a plain host compiler.
#pragma once
#if defined( __HIPCC__ )
#include <hip/hip_runtime.h>
#define TMC2_SORT_FN __host__ __device__
#else
#define TMC2_SORT_FN
#endif

namespace tmc2 {

// The reference orders a target's backward candidates with std::sort( ..., dist < dist ): libstdc++'s introsort
// (median-of-3 quicksort down to 16-element runs, then one insertion sort).  It is not stable, so for equal
// distances the outcome depends on the algorithm's exact moves -- reproduced here move for move on the list that
// is first brought into source-index order (the order in which the reference appended the candidates).
// E: an entry with the distance in .x (uint2 on the device; the host restatement of the transfer sorts its own pairs).
template <typename E>
struct CandSortOf {
  E* a;
  TMC2_SORT_FN bool less( int i, int j ) const { return a[i].x < a[j].x; }
  TMC2_SORT_FN void swap( int i, int j ) const {
    const E t = a[i];
    a[i]          = a[j];
    a[j]          = t;
  }
  TMC2_SORT_FN void unguardedLinearInsert( int last ) const {
    const E val  = a[last];
    int         next = last - 1;
    while ( val.x < a[next].x ) {
      a[last] = a[next];
      last    = next;
      --next;
    }
    a[last] = val;
  }
  TMC2_SORT_FN void insertionSort( int first, int last ) const {
    for ( int i = first + 1; i < last; ++i ) {
      if ( a[i].x < a[first].x ) {
        const E val = a[i];
        for ( int k = i; k > first; --k ) a[k] = a[k - 1];
        a[first] = val;
      } else {
        unguardedLinearInsert( i );
      }
    }
  }
  TMC2_SORT_FN void moveMedianToFirst( int result, int x, int y, int z ) const {
    if ( less( x, y ) ) {
      if ( less( y, z ) )
        swap( result, y );
      else if ( less( x, z ) )
        swap( result, z );
      else
        swap( result, x );
    } else if ( less( x, z ) )
      swap( result, x );
    else if ( less( y, z ) )
      swap( result, z );
    else
      swap( result, y );
  }
  TMC2_SORT_FN int unguardedPartition( int first, int last, int pivot ) const {
    for ( ;; ) {
      while ( less( first, pivot ) ) ++first;
      --last;
      while ( less( pivot, last ) ) --last;
      if ( !( first < last ) ) return first;
      swap( first, last );
      ++first;
    }
  }
  // returns false if the depth limit was reached (libstdc++ would switch to heapsort; not reproduced)
  TMC2_SORT_FN bool sort( int n ) const {
    if ( n < 2 ) return true;
    int lg = 0;
    while ( ( n >> ( lg + 1 ) ) > 0 ) ++lg;
    // __introsort_loop: recursion on the right part, iteration on the left -> explicit stack of right parts
    int  stackFirst[64], stackLast[64], stackDepth[64], sp = 0;
    int  first = 0, last = n, depth = 2 * lg;
    bool ok = true;
    for ( ;; ) {
      while ( last - first > 16 ) {
        if ( depth == 0 ) {
          ok = false;
          break;
        }
        --depth;
        const int mid = first + ( last - first ) / 2;
        moveMedianToFirst( first, first + 1, mid, last - 1 );
        const int cut = unguardedPartition( first + 1, last, first );
        // the reference recurses into [cut,last) FIRST and then continues with [first,cut); the two ranges are
        // disjoint, so the order in which they are processed does not change the result
        if ( sp < 64 ) {
          stackFirst[sp] = cut, stackLast[sp] = last, stackDepth[sp] = depth;
          ++sp;
        } else {
          ok = false;
        }
        last = cut;
      }
      if ( sp == 0 ) break;
      --sp;
      first = stackFirst[sp], last = stackLast[sp], depth = stackDepth[sp];
    }
    // __final_insertion_sort
    if ( n > 16 ) {
      insertionSort( 0, 16 );
      for ( int i = 16; i < n; ++i ) unguardedLinearInsert( i );
    } else {
      insertionSort( 0, n );
    }
    return ok;
  }
};
#if defined( __HIPCC__ )
using CandSort = CandSortOf<uint2>;
#endif

}  // namespace tmc2
