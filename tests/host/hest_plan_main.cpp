// Stand-alone driver of the channel-estimate capture's call plan (csrc/hest_plan.hpp) for tests/test_hest_plan_host.py, built with
// the host sanitizers.  Every line of standard input is one question: a command and `key=value` tokens (a missing key is 0).
//   shape keys: nfft t_guard n_symb n_carrier np nd bps frame_words f64 pilots_in_band device ctx_device
//   capture <shape> time_desync= freq_desync= study= bins_n= bins_lo= bins_hi= out=  -> the capture checks alone
//   rx      plan=0|1 <shape> rx= f64_flag= n_frames= time_desync= freq_desync= out=  -> hest_rx_prelude
//   study   plan=0|1 <shape> f64_flag= frame0= n_points= fpp= max_chunk= points=0|1 sto_mode= cfo_mode= reg=none|15 digits
//           h=none|bad|N (N unit taps) taps=none|delays,.. power= (every tap's) time_desync= freq_desync= bins_n= bins_lo= bins_hi= out=
//                                                                                    -> hest_study_prelude
//   chunk   <shape> scr= imp= fade_taps= fpp= cap=                                   -> frames per chunk, bytes per frame, row bytes
//   pass    <shape> frames=         -> threads lanes frames_per_wg lds grid acc_threads acc_grid acc_grid_pilots acc_lds
//   table   n= lo= hi= n_carrier=                                                    -> the n + 1 thresholds, as %a
//   bin     n= lo= hi= n_carrier= v= (hexadecimal or decimal floating point)         -> the bin of v on that table
//   binat   n= lo= hi= n_carrier= edge= side=-1|0|1                                  -> the bin of the value just below / at / just
//                                                                                       above threshold `edge`
// A refusal answers `refused <id> <message>`.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../ofdm-course_amd/csrc/hest_plan.hpp"

using namespace ofdm;

static const char* const IDS[HEST_REFUSALS] = {
    "ok", "args", "device", "precision", "no_data", "pilots", "nfft", "stream", "modes", "sc_ref", "channel", "tap_delay",
    "tap_count", "fade_count", "fade_missing", "fade_delay", "fade_twice", "fade_power", "register", "descr_needed",
    "descr_unwanted", "points_missing", "points_many", "mmse_points", "mmse_fading", "chunk_cap", "mer_skip", "nmse_mp",
    "frames", "both", "time_desync", "freq_desync", "pilots", "route", "bins", "output"};

typedef std::map<std::string, std::string> KV;

static long long num(const KV& kv, const char* k) {
  const auto it = kv.find(k);
  return it == kv.end() ? 0 : std::atoll(it->second.c_str());
}
static double real(const KV& kv, const char* k) {
  const auto it = kv.find(k);
  return it == kv.end() ? 0.0 : std::strtod(it->second.c_str(), nullptr);
}
static std::string str(const KV& kv, const char* k, const char* dflt = "") {
  const auto it = kv.find(k);
  return it == kv.end() ? dflt : it->second;
}

static TxfShape shape(const KV& kv) {
  TxfShape s{};
  s.nfft = (int)num(kv, "nfft"); s.t_guard = (int)num(kv, "t_guard"); s.n_symb = (int)num(kv, "n_symb");
  s.n_carrier = (int)num(kv, "n_carrier"); s.np = (int)num(kv, "np"); s.nd = (int)num(kv, "nd"); s.bps = (int)num(kv, "bps");
  s.frame_words = (int)num(kv, "frame_words"); s.f64 = (int)num(kv, "f64"); s.pilots_in_band = (int)num(kv, "pilots_in_band");
  s.device = (int)num(kv, "device"); s.ctx_device = (int)num(kv, "ctx_device");
  return s;
}

static HestCapture capture(const KV& kv, bool study) {
  HestCapture c;
  c.time_desync = (int)num(kv, "time_desync"); c.freq_desync = (int)num(kv, "freq_desync"); c.study = study;
  c.bins.n = (int)num(kv, "bins_n"); c.bins.lo = real(kv, "bins_lo"); c.bins.hi = real(kv, "bins_hi");
  c.out = num(kv, "out") != 0;
  return c;
}

static std::vector<double> table(const KV& kv) {
  HestBins b;
  b.n = (int)num(kv, "n"); b.lo = real(kv, "lo"); b.hi = real(kv, "hi");
  std::vector<double> thr((size_t)b.n + 1);
  hest_thresholds(b, (int)num(kv, "n_carrier"), thr.data());
  return thr;
}

static int answer(int id, const TxfWhy& w) {
  if (id < 0 || id >= HEST_REFUSALS) { std::fprintf(stderr, "bad id %d\n", id); return 3; }
  if (id != TXF_OK) std::printf("refused %s %s\n", IDS[id], w.text);
  else std::printf("ok\n");
  return 0;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    in >> cmd;
    KV kv;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) { std::fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
      kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    const TxfShape s = shape(kv);
    TxfWhy w;
    if (cmd == "capture") {
      if (const int rc = answer(hest_check_capture(s, capture(kv, num(kv, "study") != 0), "rx_hest", w), w)) return rc;
    } else if (cmd == "rx") {
      if (const int rc = answer(hest_rx_prelude(num(kv, "plan") ? &s : nullptr, num(kv, "rx") != 0, num(kv, "f64_flag") != 0,
                                                num(kv, "n_frames"), capture(kv, false), w), w))
        return rc;
    } else if (cmd == "study") {
      std::vector<uint8_t> reg;
      const std::string r = str(kv, "reg", "none");
      if (r != "none") for (char ch : r) reg.push_back((uint8_t)(ch - '0'));
      const std::string hs = str(kv, "h", "none"), ts = str(kv, "taps", "none");
      std::vector<double> h;                                       // complex double or float pairs, read in the plan's precision
      std::vector<float> hf;
      if (hs != "none" && hs != "bad")
        for (long long i = 0; i < std::atoll(hs.c_str()); ++i) { h.push_back(1.0); h.push_back(0.0); hf.push_back(1.0f); hf.push_back(0.0f); }
      std::vector<int32_t> delay;
      std::vector<double> power;
      if (ts != "none") {
        std::istringstream tin(ts);
        std::string d;
        while (std::getline(tin, d, ',')) { delay.push_back((int32_t)std::atoll(d.c_str())); power.push_back(real(kv, "power")); }
      }
      const std::vector<double> snr(1, 20.0);
      const std::vector<uint64_t> seeds(1, 1);
      TxfCall c("hest_study", num(kv, "frame0"), num(kv, "fpp"), r == "none" ? nullptr : reg.data());
      c.plan = num(kv, "plan") ? &s : nullptr;
      c.f64_flag = num(kv, "f64_flag") != 0;
      const bool points = num(kv, "points") != 0;
      c.with_points(points ? snr.data() : nullptr, points ? seeds.data() : nullptr, num(kv, "n_points"), num(kv, "max_chunk"));
      c.with_imp((int)num(kv, "sto_mode"), (int)num(kv, "cfo_mode"));
      const bool fading = ts != "none";
      const void* hp = hs == "none" ? nullptr : hs == "bad" ? nullptr : s.f64 ? (const void*)h.data() : (const void*)hf.data();
      const int h_len = hs == "none" ? 0 : hs == "bad" ? 3 : (int)(h.size() / 2);
      if (fading) c.with_fading(delay.data(), power.data(), (int)delay.size());
      else c.with_h(hp, h_len);
      TxfChannel ch;
      TxfGains g;
      if (const int rc = answer(hest_study_prelude(c, fading && hs != "none", capture(kv, true), ch, g, w), w)) return rc;
    } else if (cmd == "chunk") {
      const TxfUse u = sync_use(num(kv, "scr") != 0, num(kv, "imp") != 0, (int)num(kv, "fade_taps"));
      std::printf("%lld %zu %zu\n", (long long)hest_chunk(s, u, num(kv, "fpp"), num(kv, "cap")), txf_frame_bytes(s, u), hest_row_bytes(s));
    } else if (cmd == "pass") {
      const HestPass p = hest_pass(s, num(kv, "frames"));
      std::printf("%d %d %d %zu %u %d %u %u %zu\n", p.threads, p.lanes, p.frames_per_wg, p.lds, p.grid, p.acc_threads, p.acc_grid,
                  p.acc_grid_pilots, p.acc_lds);
    } else if (cmd == "table") {
      const std::vector<double> thr = table(kv);
      for (size_t i = 0; i < thr.size(); ++i) std::printf(i ? " %a" : "%a", thr[i]);
      std::printf("\n");
    } else if (cmd == "bin") {
      const std::vector<double> thr = table(kv);
      std::printf("%d\n", hest_bin(real(kv, "v"), thr.data(), (int)thr.size() - 1));
    } else if (cmd == "binat") {
      const std::vector<double> thr = table(kv);
      const double e = thr[(size_t)num(kv, "edge")];
      const long long side = num(kv, "side");
      const double v = side < 0 ? std::nextafter(e, -std::numeric_limits<double>::infinity())
                                : side > 0 ? std::nextafter(e, std::numeric_limits<double>::infinity()) : e;
      std::printf("%d\n", hest_bin(v, thr.data(), (int)thr.size() - 1));
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
