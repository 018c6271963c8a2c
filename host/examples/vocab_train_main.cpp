// Training a vocabulary on the mirror: x::VocabularyTrainer (DBoW3::Vocabulary::create, third_party/DBow3/src/Vocabulary.cpp:
// 157-186) on descriptors read from a file, in the pieces the file gives; the tree arrays and the outcome printed.
//   usage  : xk_vocab_train_example case.txt
//   case   : k L desc_bytes seed max_iter n_pieces, then per piece: n  b0 b1 ... (n rows of desc_bytes bytes)
//   output : V k L n_nodes kmax desc_bytes n_words
//            D ...   node_desc   [n_nodes][desc_bytes]
//            C ...   children    [n_nodes][kmax]
//            W ...   word_of_node [n_nodes]
//            N ...   node_of_word [n_words]
//            O levels capped_nodes launches host_waits  nodes passes (per level, L pairs)
//   The V / D / C / W / N lines, without their letters, are the vocabulary file xk_describe_example reads.
#include <cstdio>
#include <fstream>

#include "x/place_recognition/database.h"

using namespace x;

template <class T>
static void print_line(const char *tag, const std::vector<T> &v) {
  std::printf("%s", tag);
  for (const T &x : v) std::printf(" %d", (int)x);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s case.txt\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  int k, L, desc_bytes, max_iter, n_pieces;
  unsigned long seed;
  in >> k >> L >> desc_bytes >> seed >> max_iter >> n_pieces;
  if (!in || desc_bytes < 1 || n_pieces < 0) { std::fprintf(stderr, "bad case file\n"); return 2; }
  std::vector<Descriptors> pieces((size_t)n_pieces);
  int total = 0;
  for (Descriptors &d : pieces) {
    in >> d.rows;
    if (!in || d.rows < 0) { std::fprintf(stderr, "bad case file\n"); return 2; }
    d.cols = desc_bytes;
    d.data.resize((size_t)d.rows * desc_bytes);
    for (auto &b : d.data) { int t; in >> t; b = (unsigned char)t; }
    total += d.rows;
  }
  if (!in) { std::fprintf(stderr, "bad case file\n"); return 2; }
  xk_handle *xk = nullptr;
  if (xk_create(0, 4, 0, 4, &xk) != XK_OK) { std::fprintf(stderr, "xk_create failed\n"); return 1; }
  int rc = 0;
  try {
    VocabularyTrainer trainer(xk, k, L, desc_bytes, total > 0 ? total : 1);
    for (const Descriptors &d : pieces) trainer.add(d);
    VocabularyTrainer::Outcome oc;
    const PRVocabulary v = trainer.train(seed, max_iter, &oc);
    std::printf("V %d %d %d %d %d %zu\n", v.k, v.L, v.nNodes(), v.kmax, v.desc_bytes, v.node_of_word.size());
    print_line("D", v.node_desc);
    print_line("C", v.children);
    print_line("W", v.word_of_node);
    print_line("N", v.node_of_word);
    std::printf("O %d %d %d %d", oc.levels, oc.capped_nodes, oc.launches, oc.host_waits);
    for (int l = 0; l < L; ++l) std::printf(" %d %d", oc.level_nodes[l], oc.level_passes[l]);
    std::printf("\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    rc = 1;
  }
  xk_destroy(xk);
  return rc;
}
