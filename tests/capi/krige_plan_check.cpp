// The pure part of the kriging level plan (hmsc_amd/csrc/krige_level.h) as a stand-alone host program:
// pair grouping, mode checks and the two device-memory needs, printed for the specs given on stdin.
// It calls no HIP function.  tests/test_host_krige_plan.py builds it with the library's flags plus
// -fsanitize=address,undefined, runs it and holds the output to a restatement of the formulas.
//
// One spec per line:
//   keep_zero slab mode np nn sDim nK nNeighbours G S nf coords dist knots | alphas (G) | alpha (S * nf)
// coords / dist / knots: 1 = given (the functions look at the pointer only).
#include <cstdio>
#include <iostream>
#include <sstream>

#include "../../hmsc_amd/csrc/krige_level.h"

using namespace hmsc;

template <class T>
static void row(const char* name, const std::vector<T>& v) {
  std::ostringstream o;
  o.precision(17);
  o << name;
  for (const T& x : v) o << ' ' << x;
  std::puts(o.str().c_str());
}

int main() {
  static const double some = 0.0;  // a non-null place for the geometry pointers
  std::string text;
  while (std::getline(std::cin, text)) {
    std::istringstream in(text);
    int keep_zero, has_coords, has_dist, has_knots;
    size_t slab;
    char bar;
    KrigeSpec q{};
    in >> keep_zero >> slab >> q.mode >> q.np >> q.nn >> q.sDim >> q.nK >> q.nNeighbours >> q.G >> q.S >> q.nf >>
        has_coords >> has_dist >> has_knots >> bar;
    std::vector<double> alphas(q.G);
    for (double& a : alphas) in >> a;
    in >> bar;
    std::vector<int32_t> alpha((size_t)q.S * q.nf);
    for (int32_t& g : alpha) in >> g;
    if (!in) {
      std::puts("bad spec");
      return 2;
    }
    q.coords = has_coords ? &some : nullptr, q.dist = has_dist ? &some : nullptr, q.knots = has_knots ? &some : nullptr;
    q.alphas = alphas.data(), q.alpha = alpha.data();
    std::puts("spec");
    try {
      // hmsc_krige checks the mode's arguments first; the map once a group needs them
      if (keep_zero) krige_check_mode(q, "check: ");
      const KrigeGroups g = krige_group_pairs(q, keep_zero != 0, "check: ");
      if (!keep_zero && g.size() > 0) krige_check_mode(q, "check: ");
      row("g_idx", g.g_idx);
      row("g_alpha", g.g_alpha);
      row("g_off", g.g_off);
      row("col_s", g.col_s);
      row("col_h", g.col_h);
      row("zflag", g.zflag);
      std::printf("cmax %zu\n", g.cmax);
      // one-shot: hmsc_krige's plan; resident: a map level's, serving at most `slab` new units at a time
      const unsigned long long need = krige_need_bytes(q, g, !keep_zero, keep_zero ? (size_t)q.nn : slab);
      std::printf("need %llu\n", need);
    } catch (const HmscError& e) {
      std::printf("refused %s\n", e.what());
    }
  }
  return 0;
}
