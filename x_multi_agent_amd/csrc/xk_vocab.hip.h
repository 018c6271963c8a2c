// xk_vocab.hip.h -- training of a DBoW3 vocabulary tree for binary descriptors on the device (gfx950): hierarchical k-means
// with k-means++ seeding, Hamming distances and bit-majority means.
//
//   DBoW3::Vocabulary::create            third_party/DBow3/src/Vocabulary.cpp:157-186
//   HKmeansStep                          :233-394     (trivial node, Lloyd loop, convergence, recursion)
//   initiateClustersKMpp                 :409-491     (first centre uniform, later ones by the running sum of min_dist)
//   DescManip::meanValue, binary branch  DescManip.cpp:26-75
//
// The tree is built level by level, not by recursion.  A level is a list of nodes, each a contiguous range of the level's
// permutation `perm` (original descriptor indices, sorted by (node, original index): the order within a node is the input
// order the running sums and the trivial case depend on).  All nodes of a level run their seeding steps and Lloyd passes in
// the same launches; a node's draws depend on (seed, path code, step) only, so this gives the tree of the recursive
// definition (tests/vocab_np.py).  Everything is integer work: sums by integer atomics and scans, so neither the order of
// addition nor the split of a scan into workgroups can show in the result.
//
//   xk_voc_seed_first      first centre of every node; a trivial node (cnt <= k) gets one centre per descriptor
//   xk_voc_seed_dist       min_dist against the node's newest centre, workgroup sums
//   xk_voc_scan_u64        exclusive scan of the workgroup sums (one workgroup)
//   xk_voc_prefix          inclusive 64-bit running sum of min_dist over the whole level
//   xk_voc_seed_pick       per node: dist_sum and cut from the running sums at its ends, the one position whose running
//                          sum reaches the cut becomes the next centre
//   xk_voc_assoc           nearest centre (strict '<': lowest index wins), changed count per node
//   xk_voc_status          per node: converged / capped / goes on; the level's record for the host
//   xk_voc_majority_count  per (node, cluster) bit counters: wavefront ballots per bit, one integer atomic per counter and wave
//   xk_voc_majority_set    threshold  count >= n/2 + n%2;  an empty group leaves its centre
//   xk_voc_hist            per (node, cluster) sizes, per workgroup cluster histogram
//   xk_voc_scan_hist       exclusive scan of the histogram columns (one workgroup)
//   xk_voc_scatter         stable partition of every node's range by cluster into the next level's permutation
//
// Descriptors are little-endian 32-bit words (desc_bytes % 4 == 0, <= 64 bytes), as in xk_place.hip.h.  The majority rule
// works bit by bit, so DBoW3's MSB-first bit numbering inside a byte does not enter.
#pragma once
#include <hip/hip_runtime.h>
#include "xk_place.hip.h"
#include "xk_ransac.hip.h"

#define XK_VOC_KMAX 16        // k <= 16
#define XK_VOC_LMAX 8         // L <= 8
#define XK_VOC_T 256          // workgroup size of every kernel here
#define XK_VOC_LDS_WORDS 4096 // centre words a workgroup of xk_voc_assoc stages (16 KB)

struct XkVocNode {            // one node of the level being split
  int start, cnt;             // its range of the level's permutation
  int ncent;                  // centres chosen so far (seeding), then the number of its children
  int state;                  // 1 while its Lloyd loop runs; 0: trivial, converged or capped
  int changed;                // descriptors whose cluster changed in the latest association pass
  int pad;
  unsigned long long key;     // K = sm(seed ^ sm(path code))
};

struct XkVocLevel {
  const unsigned int *desc;   // [N][W] all training descriptors, in the order they were added
  int W, k, M, A;             // words per descriptor, branching, positions and nodes of this level
  const int *perm;            // [M] original index of every position
  const int *node_of_pos;     // [M] non-decreasing
  XkVocNode *nodes;           // [A]
  unsigned int *cen;          // [A][k][W]
  int *assoc;                 // [M]
  int *min_dist;              // [M]
  unsigned long long *prefix; // [M] inclusive running sum of min_dist
  unsigned long long *bsum;   // [workgroups]
  int *cnt;                   // [A][k][32 W] majority counters, zero between passes
  int *gsize;                 // [A][k] group sizes of the latest majority count
  int *csize;                 // [A][k] group sizes of the final association (xk_voc_hist)
  int *hist;                  // [workgroups][k]
  unsigned long long *rec;    // cumulative over the training: nodes that went on, nodes capped, changed associations
};

// Exclusive scan over the workgroup (256 threads); returns the exclusive value, *total = the workgroup's sum.
template <class T>
__device__ __forceinline__ T xk_voc_block_scan(T v, T *total) {
  __shared__ T s_w[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();                              // (s_w of an earlier call has been read)
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  T off = 0;
  for (int j = 0; j < w; ++j) off += s_w[j];
  *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  return off + inc - v;
}

// The node of a position, -1 for anything that is not a node of this level (a position the split did not fill).
__device__ __forceinline__ int xk_voc_node_at(const XkVocLevel &lv, int pos) {
  const int a = lv.node_of_pos[pos];
  return (unsigned int)a < (unsigned int)lv.A ? a : -1;
}

__device__ __forceinline__ void xk_voc_load(const XkVocLevel &lv, int pos, unsigned int d[XK_PR_MAXW]) {
  const unsigned int *p = lv.desc + (size_t)lv.perm[pos] * lv.W;
#pragma unroll
  for (int w = 0; w < XK_PR_MAXW; ++w) d[w] = (w < lv.W) ? p[w] : 0u;
}

__device__ __forceinline__ int xk_voc_ham(const unsigned int d[XK_PR_MAXW], const unsigned int *c, int W) {
  int dist = 0;
#pragma unroll
  for (int w = 0; w < XK_PR_MAXW; ++w)
    if (w < W) dist += __popc(d[w] ^ c[w]);
  return dist;
}

// The first level: every descriptor in input order, all in node 0 (getFeatures, :220-228).
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_iota(int *perm, int *node_of_pos, int n) {
  const int i = blockIdx.x * XK_VOC_T + threadIdx.x;
  if (i < n) { perm[i] = i; node_of_pos[i] = 0; }
}

// One thread per node.  Vocabulary.cpp:248-258 (trivial case) and :433-436 (first centre).
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_seed_first(XkVocLevel lv) {
  const int a = blockIdx.x * XK_VOC_T + threadIdx.x;
  if (a >= lv.A) return;
  XkVocNode nd = lv.nodes[a];
  unsigned int *cen = lv.cen + (size_t)a * lv.k * lv.W;
  if (nd.cnt <= lv.k) {
    for (int i = 0; i < nd.cnt; ++i) {
      const unsigned int *p = lv.desc + (size_t)lv.perm[nd.start + i] * lv.W;
      for (int w = 0; w < lv.W; ++w) cen[i * lv.W + w] = p[w];
      lv.assoc[nd.start + i] = i;
    }
    lv.nodes[a].ncent = nd.cnt;
  } else {
    const int first = (int)(xk_ransac_mix(nd.key) % (unsigned long long)nd.cnt);
    const unsigned int *p = lv.desc + (size_t)lv.perm[nd.start + first] * lv.W;
    for (int w = 0; w < lv.W; ++w) cen[w] = p[w];
    lv.nodes[a].ncent = 1;
  }
}

// Seeding step j (1 ... k-1), one thread per position: min_dist against centre j-1 of the node (:441-457).  A node that is
// trivial or whose seeding has stopped (ncent < j: its min_dist are all zero) keeps what it has.
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_seed_dist(XkVocLevel lv, int j) {
  const int pos = blockIdx.x * XK_VOC_T + threadIdx.x;
  unsigned long long m = 0;
  if (pos < lv.M) {
    const int a = xk_voc_node_at(lv, pos);
    const XkVocNode nd = lv.nodes[max(a, 0)];
    int v = (j == 1) ? 0 : lv.min_dist[pos];
    if (a >= 0 && nd.state && nd.ncent == j) {
      unsigned int d[XK_PR_MAXW];
      xk_voc_load(lv, pos, d);
      const int dist = xk_voc_ham(d, lv.cen + ((size_t)a * lv.k + (j - 1)) * lv.W, lv.W);
      v = (j == 1) ? dist : min(v, dist);
    }
    lv.min_dist[pos] = v;
    m = (unsigned long long)v;
  }
  unsigned long long total;
  xk_voc_block_scan(m, &total);
  if (threadIdx.x == 0) lv.bsum[blockIdx.x] = total;
}

// In place exclusive scan of v[0 .. n), one workgroup, chunks of 256 with a running base.
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_scan_u64(unsigned long long *v, int n) {
  unsigned long long base = 0;
  for (int i0 = 0; i0 < n; i0 += XK_VOC_T) {
    const int i = i0 + threadIdx.x;
    const unsigned long long x = i < n ? v[i] : 0ull;
    unsigned long long total;
    const unsigned long long ex = xk_voc_block_scan(x, &total);
    if (i < n) v[i] = base + ex;
    base += total;
  }
}

__global__ __launch_bounds__(XK_VOC_T) void xk_voc_prefix(XkVocLevel lv) {
  const int pos = blockIdx.x * XK_VOC_T + threadIdx.x;
  const unsigned long long m = pos < lv.M ? (unsigned long long)lv.min_dist[pos] : 0ull;
  unsigned long long total;
  const unsigned long long ex = xk_voc_block_scan(m, &total);
  if (pos < lv.M) lv.prefix[pos] = lv.bsum[blockIdx.x] + ex + m;
}

// Seeding step j, one thread per position (:460-485): dist_sum of the node from the running sums at its two ends,
// cut = 1 + sm(K + j) mod dist_sum; the first position whose inclusive running sum reaches the cut is the one with
// exclusive sum < cut <= inclusive sum -- exactly one thread per node, which writes centre j.  Only that thread writes
// nodes[a].ncent, and it read j there; whoever reads j + 1 instead leaves.
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_seed_pick(XkVocLevel lv, int j) {
  const int pos = blockIdx.x * XK_VOC_T + threadIdx.x;
  if (pos >= lv.M) return;
  const int a = xk_voc_node_at(lv, pos);
  if (a < 0) return;
  const XkVocNode nd = lv.nodes[a];
  if (!nd.state || nd.ncent != j) return;
  const unsigned long long base = nd.start > 0 ? lv.prefix[nd.start - 1] : 0ull;
  const unsigned long long sum = lv.prefix[nd.start + nd.cnt - 1] - base;
  if (sum == 0ull) return;                                    // every descriptor equals a centre: seeding stops (:486-487)
  const unsigned long long cut = 1ull + xk_ransac_mix(nd.key + (unsigned long long)j) % sum;
  const unsigned long long inc = lv.prefix[pos] - base, exc = inc - (unsigned long long)lv.min_dist[pos];
  if (exc < cut && cut <= inc) {
    const unsigned int *p = lv.desc + (size_t)lv.perm[pos] * lv.W;
    unsigned int *c = lv.cen + ((size_t)a * lv.k + j) * lv.W;
    for (int w = 0; w < lv.W; ++w) c[w] = p[w];
    lv.nodes[a].ncent = j + 1;
  }
}

// Association pass (:307-326), one thread per position.  The centres of the nodes a workgroup touches (node_of_pos is
// non-decreasing, so they are one contiguous block of cen) go through LDS when they fit.
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_assoc(XkVocLevel lv, int pass) {
  __shared__ unsigned int s_cen[XK_VOC_LDS_WORDS];
  const int pos0 = blockIdx.x * XK_VOC_T, pos = pos0 + threadIdx.x;
  const int a0 = xk_voc_node_at(lv, pos0), a1 = xk_voc_node_at(lv, min(pos0 + XK_VOC_T, lv.M) - 1);
  const int row_words = lv.k * lv.W;
  const long long words = (long long)(a1 - a0 + 1) * row_words;
  const bool staged = a0 >= 0 && a1 >= a0 && words <= XK_VOC_LDS_WORDS;
  if (staged) {
    const unsigned int *src = lv.cen + (size_t)a0 * row_words;
    for (int i = threadIdx.x; i < (int)words; i += XK_VOC_T) s_cen[i] = src[i];
  }
  __syncthreads();
  bool changed = false;
  int a = -1;
  if (pos < lv.M) {
    a = xk_voc_node_at(lv, pos);
    const XkVocNode nd = lv.nodes[max(a, 0)];
    if (a >= 0 && nd.state) {
      unsigned int d[XK_PR_MAXW];
      xk_voc_load(lv, pos, d);
      const unsigned int *c = (staged && a >= a0 && a <= a1) ? s_cen + (size_t)(a - a0) * row_words : lv.cen + (size_t)a * row_words;
      int best = xk_voc_ham(d, c, lv.W), bc = 0;
      for (int q = 1; q < nd.ncent; ++q) {
        const int dist = xk_voc_ham(d, c + q * lv.W, lv.W);
        if (dist < best) { best = dist; bc = q; }
      }
      changed = pass > 1 && lv.assoc[pos] != bc;
      lv.assoc[pos] = bc;
    }
  }
  // one atomic per wavefront where its changed lanes share a node, else one per lane
  const unsigned long long cm = __ballot(changed);
  if (cm) {
    const int leader = __ffsll((long long)cm) - 1;
    const int la = __shfl(a, leader, 64);
    const bool uniform = __ballot(changed && a != la) == 0ull;
    if (uniform) {
      if ((threadIdx.x & 63) == leader) atomicAdd(&lv.nodes[la].changed, __popcll(cm));
    } else if (changed) {
      atomicAdd(&lv.nodes[a].changed, 1);
    }
  }
}

// After association pass `pass`, one thread per node (:331-354): the first association is never compared; from the second
// on the node ends when nothing changed; at max_iter it ends as capped.  A node that goes on gets its group sizes zeroed
// for the majority count that follows.
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_status(XkVocLevel lv, int pass, int max_iter) {
  const int a = blockIdx.x * XK_VOC_T + threadIdx.x;
  if (a >= lv.A) return;
  if (!lv.nodes[a].state) return;
  const int ch = lv.nodes[a].changed;
  lv.nodes[a].changed = 0;
  if (ch) atomicAdd(lv.rec + 2, (unsigned long long)ch);
  if (pass > 1 && ch == 0) {
    lv.nodes[a].state = 0;
  } else if (pass >= max_iter) {
    lv.nodes[a].state = 0;
    atomicAdd(lv.rec + 1, 1ull);
  } else {
    atomicAdd(lv.rec + 0, 1ull);
    for (int c = 0; c < lv.k; ++c) lv.gsize[(size_t)a * lv.k + c] = 0;
  }
}

// Bit counters of every (node, cluster) group of the nodes that go on (DescManip.cpp:43-59).  A wavefront takes 64
// positions and works through the distinct groups among them: per bit one ballot of the group's lanes, lane (bit mod 64)
// keeps the count, then one integer atomic per counter.
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_majority_count(XkVocLevel lv) {
  const int pos = blockIdx.x * XK_VOC_T + threadIdx.x, lane = threadIdx.x & 63;
  int key = -1;
  unsigned int d[XK_PR_MAXW];
#pragma unroll
  for (int w = 0; w < XK_PR_MAXW; ++w) d[w] = 0u;
  if (pos < lv.M) {
    const int a = xk_voc_node_at(lv, pos);
    if (a >= 0 && lv.nodes[a].state) {
      key = a * lv.k + lv.assoc[pos];
      xk_voc_load(lv, pos, d);
    }
  }
  const int bits = 32 * lv.W;
  unsigned long long rem = __ballot(key >= 0);
  while (rem) {
    const int leader = __ffsll((long long)rem) - 1;
    const int kk = __shfl(key, leader, 64);
    const bool mine = key == kk;
    const unsigned long long mm = __ballot(mine);
    rem &= ~mm;
    int acc[XK_PR_MAXW / 2];
#pragma unroll
    for (int j = 0; j < XK_PR_MAXW / 2; ++j) acc[j] = 0;
#pragma unroll
    for (int w = 0; w < XK_PR_MAXW; ++w)
      if (w < lv.W) {
#pragma unroll
        for (int b = 0; b < 32; ++b) {
          const int c = __popcll(__ballot(mine && ((d[w] >> b) & 1u)));
          if (lane == (w & 1) * 32 + b) acc[w >> 1] = c;
        }
      }
#pragma unroll
    for (int j = 0; j < XK_PR_MAXW / 2; ++j) {
      const int bit = j * 64 + lane;
      if (bit < bits && acc[j]) atomicAdd(&lv.cnt[(size_t)kk * bits + bit], acc[j]);
    }
    if (lane == 0) atomicAdd(&lv.gsize[kk], __popcll(mm));
  }
}

// One thread per (node, cluster, word) (DescManip.cpp:30-36, :64-74): bit set iff count >= n/2 + n%2; n = 1 gives the
// descriptor itself, n = 0 leaves the centre.  The counters go back to zero.
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_majority_set(XkVocLevel lv) {
  const long long t = (long long)blockIdx.x * XK_VOC_T + threadIdx.x;
  if (t >= (long long)lv.A * lv.k * lv.W) return;
  const int w = (int)(t % lv.W);
  const int g = (int)(t / lv.W), a = g / lv.k, c = g % lv.k;
  const XkVocNode nd = lv.nodes[a];
  if (!nd.state || c >= nd.ncent) return;
  const int n = lv.gsize[g];
  if (n == 0) return;
  const int thr = n / 2 + n % 2;
  int *cnt = lv.cnt + ((size_t)g * lv.W + w) * 32;
  unsigned int word = 0u;
#pragma unroll
  for (int b = 0; b < 32; ++b) {
    if (cnt[b] >= thr) word |= 1u << b;
    cnt[b] = 0;
  }
  lv.cen[(size_t)g * lv.W + w] = word;
}

// Sizes of the final groups and the workgroup's histogram over the cluster index, one thread per position.
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_hist(XkVocLevel lv) {
  __shared__ int s_h[XK_VOC_KMAX];
  if (threadIdx.x < XK_VOC_KMAX) s_h[threadIdx.x] = 0;
  __syncthreads();
  const int pos = blockIdx.x * XK_VOC_T + threadIdx.x, lane = threadIdx.x & 63;
  int key = -1, c = -1;
  if (pos < lv.M) {
    const int a = xk_voc_node_at(lv, pos);
    c = lv.assoc[pos];
    if (a >= 0 && c >= 0 && c < lv.k) key = a * lv.k + c;
  }
  unsigned long long rem = __ballot(key >= 0);
  while (rem) {
    const int leader = __ffsll((long long)rem) - 1;
    const int kk = __shfl(key, leader, 64);
    const unsigned long long mm = __ballot(key == kk);
    rem &= ~mm;
    if (lane == leader) {
      atomicAdd(&lv.csize[kk], __popcll(mm));
      atomicAdd(&s_h[c], __popcll(mm));
    }
  }
  __syncthreads();
  if (threadIdx.x < lv.k) lv.hist[(size_t)blockIdx.x * lv.k + threadIdx.x] = s_h[threadIdx.x];
}

// In place exclusive scan of every column of hist [nb][k], one workgroup.
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_scan_hist(int *hist, int nb, int k) {
  for (int c = 0; c < k; ++c) {
    int base = 0;
    for (int i0 = 0; i0 < nb; i0 += XK_VOC_T) {
      const int i = i0 + threadIdx.x;
      const int x = i < nb ? hist[(size_t)i * k + c] : 0;
      int total;
      const int ex = xk_voc_block_scan(x, &total);
      if (i < nb) hist[(size_t)i * k + c] = base + ex;
      base += total;
    }
  }
}

// Stable partition of every node's range by cluster (:375-392), one thread per position.  rank = positions of the level
// before this one with the same cluster index (scanned histogram + wavefront ballots); dst_off [A][k] turns it into the
// place in the next level's permutation (the host folds the child's start and the earlier nodes' sizes into it);
// child_next [A][k] is the child's node index at the next level, or -1 where the child is a leaf.
__global__ __launch_bounds__(XK_VOC_T) void xk_voc_scatter(XkVocLevel lv, const int *dst_off, const int *child_next, int *perm_next,
                                                           int *node_next, int M_next) {
  __shared__ int s_w[4][XK_VOC_KMAX];
  const int pos = blockIdx.x * XK_VOC_T + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int a = pos < lv.M ? xk_voc_node_at(lv, pos) : -1;
  int c = a >= 0 ? lv.assoc[pos] : -1;
  if (c >= lv.k) c = -1;
  int before = 0;
  for (int q = 0; q < lv.k; ++q) {
    const unsigned long long b = __ballot(c == q);
    if (c == q) before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wv][q] = __popcll(b);
  }
  __syncthreads();
  if (c < 0) return;
  int rank = lv.hist[(size_t)blockIdx.x * lv.k + c] + before;
  for (int j = 0; j < wv; ++j) rank += s_w[j][c];
  const int g = a * lv.k + c;
  const int child = child_next[g];
  if (child < 0) return;
  const int dst = dst_off[g] + rank;
  if (dst < 0 || dst >= M_next) return;                       // (cannot happen: dst counts positions of continuing children)
  perm_next[dst] = lv.perm[pos];
  node_next[dst] = child;
}
