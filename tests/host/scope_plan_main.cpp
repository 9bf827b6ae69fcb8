// Stand-alone driver of the constellation-capture plan (csrc/scope_plan.hpp) for tests/test_scope_plan_host.py, built with the
// host sanitizers.  Every line of standard input is one question, a word and `key=value` tokens:
//   iq first= count= decisions=                                  -> `ok`, or `refused <id> <message>`
//   density out= bins= half_width= skip= f64= n_carrier= decisions=
//                                                                -> `ok <grid offset> <extra bytes> <stage bytes>`, or refused
//   bin v= half_width= bins=                                     -> the bin of v (-1: not binned), scale = bins / (2 half_width)
// Numbers are read with strtod / strtoll: inf, -inf, nan, -0.0 and hexadecimal floats are accepted.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../ofdm-course_amd/csrc/scope_plan.hpp"

using namespace ofdm;

int main() {
  static const char* const IDS[SCOPE_REFUSALS] = {"ok", "iq_first", "iq_count", "iq_end", "density_out", "bins", "half_width",
                                                  "skip", "lds"};
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what, tok;
    in >> what;
    long long first = 0, count = 0, decisions = 0, skip = 0;
    int out = 0, bins = 0, f64 = 0, n_carrier = 0;
    double v = 0.0, half_width = 0.0;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) { std::fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
      const std::string k = tok.substr(0, eq), x = tok.substr(eq + 1);
      if (k == "first") first = std::strtoll(x.c_str(), nullptr, 10); else if (k == "count") count = std::strtoll(x.c_str(), nullptr, 10);
      else if (k == "decisions") decisions = std::strtoll(x.c_str(), nullptr, 10); else if (k == "skip") skip = std::strtoll(x.c_str(), nullptr, 10);
      else if (k == "out") out = std::atoi(x.c_str()); else if (k == "bins") bins = std::atoi(x.c_str());
      else if (k == "f64") f64 = std::atoi(x.c_str()); else if (k == "n_carrier") n_carrier = std::atoi(x.c_str());
      else if (k == "v") v = std::strtod(x.c_str(), nullptr); else if (k == "half_width") half_width = std::strtod(x.c_str(), nullptr);
      else { std::fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
    }
    ScopeWhy why;
    if (what == "iq" || what == "density") {
      const int id = what == "iq" ? scope_iq_check(first, count, decisions, why)
                                  : scope_density_check(out != 0, bins, half_width, skip, f64 != 0, n_carrier, decisions, why);
      if (id < 0 || id >= SCOPE_REFUSALS || (id != SCOPE_OK) != (why.text[0] != 0)) { std::fprintf(stderr, "refusal %d and its reason disagree\n", id); return 3; }
      if (id != SCOPE_OK) { std::printf("refused %s %s\n", IDS[id], why.text); continue; }
      if (what == "iq") { std::printf("ok\n"); continue; }
      std::printf("ok %zu %zu %zu\n", scope_grid_offset(f64 != 0, n_carrier, decisions), scope_lds_extra(f64 != 0, n_carrier, decisions, bins),
                  scope_stage_lds(f64 != 0, n_carrier, decisions, bins));
    } else if (what == "bin") {
      std::printf("%d\n", scope_bin(v, half_width, scope_scale(bins, half_width), bins));
    } else {
      std::fprintf(stderr, "unknown question %s\n", what.c_str());
      return 2;
    }
  }
  return 0;
}
