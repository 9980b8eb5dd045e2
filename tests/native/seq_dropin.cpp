// A scripted sequence of drop-in calls in one process, so that the state a call leaves
// (borrowed slot, shared or own plan, grown buffers, the modulator's thread-local staging)
// is what the next call meets.  tests/dropin_script.py writes the script, the payload file
// and the expected results (from the CPU oracle); tests/test_gpu_dropin_paths.py runs this
// program on the GPU and compares every line bit for bit.
//   seq_dropin <script.txt> <data.bin> <out.bin>
// Up to 8 lora_demod_workspaces (legacy helpers) and 4 lora_workspaces (workspace API).
// One operation per script line; <off> and <n> count elements in data.bin (complex64 samples
// for IQ, uint16 for symbols, from byte offset 8 * off resp. 2 * off):
//   linit  <w> <sf> <window 0|1> <max_samples> <buf|null>   lora_demod_init (scratch of max_samples, or null)
//   lfree  <w>                                              lora_demod_free
//   ldemod <w> <osr> <off> <n>                              lora_demodulate
//   lmod   <sf> <osr> <bw> <amplitude bits> <sync> <off> <n>  lora_modulate
//   init   <w> <sf> <osr> <bw> <window 0|1> <window buffer 0|1> <sync>   init
//   demod  <w> <off> <n> <cap>                              demodulate
//   est    <w> <off> <n>                                    estimate_offsets
//   comp   <w> <off> <n>                                    compensate_offsets
//   mod    <w> <off> <n> <cap>                              modulate
//   destroy <w>                                             ~lora_workspace
// One JSON line per operation: its index and name, the return value, the outputs, and the
// workspace's caller-visible device state (detail::device_state) after the call.  The
// demodulators' output arrays, *out_sync and the metrics are pre-filled with sentinels
// (kSymFill, kSyncFill, kCfoFill / kToffFill) and printed whole, so a call that must write
// nothing shows it.  Samples produced by lmod / mod / comp are appended to out.bin; the line
// names their offset and count (in samples).  The last line is the runtime's status.
#include <lora_phy/phy.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

using namespace lora_phy;
using cf = std::complex<float>;

namespace {

constexpr uint16_t kSymFill = 0xA5A5;
constexpr uint8_t kSyncFill = 0xEE;
constexpr float kCfoFill = -1234.5f, kToffFill = 4321.25f;
constexpr int kLegacy = 8, kApi = 4;

struct Legacy {
  lora_demod_workspace ws{};
  std::vector<cf> scratch;
};

struct Api {
  std::unique_ptr<lora_workspace> ws;
  std::vector<uint16_t> symbol_buf;
  std::vector<cf> fft_in, fft_out;
  std::vector<float> window;
};

uint32_t fbits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}

std::vector<unsigned char> g_data;
std::FILE* g_out = nullptr;
size_t g_out_samples = 0;

const cf* iq_at(size_t off, size_t n) {
  if (off * 8 + n * 8 > g_data.size()) {
    std::fprintf(stderr, "seq_dropin: IQ [%zu, +%zu) is outside data.bin\n", off, n);
    std::exit(2);
  }
  return reinterpret_cast<const cf*>(g_data.data() + off * 8);
}

const uint16_t* syms_at(size_t off, size_t n) {
  if (off * 2 + n * 2 > g_data.size()) {
    std::fprintf(stderr, "seq_dropin: symbols [%zu, +%zu) are outside data.bin\n", off, n);
    std::exit(2);
  }
  return reinterpret_cast<const uint16_t*>(g_data.data() + off * 2);
}

void print_state(const detail::device_state* g) {
  if (!g) {
    std::printf(", \"state\": null}\n");
    return;
  }
  std::printf(", \"state\": {\"slot\": %d, \"shared_plan\": %s, \"shared_aql\": %s, \"aql\": %s, \"aql_status\": %d, "
              "\"samples\": %zu, \"plan_osr\": %u}}\n",
              g->slot, g->shared_plan ? "true" : "false", g->shared_aql ? "true" : "false",
              g->aql ? "true" : "false", g->aql_status, g->samples, g->plan_osr);
}

void print_symbols(const std::vector<uint16_t>& s) {
  std::printf(", \"symbols\": [");
  for (size_t i = 0; i < s.size(); ++i) std::printf("%s%u", i ? ", " : "", s[i]);
  std::printf("]");
}

void append_out(const cf* x, size_t n) {
  std::printf(", \"out_off\": %zu, \"out_count\": %zu", g_out_samples, n);
  if (n && std::fwrite(x, sizeof(cf), n, g_out) != n) {
    std::fprintf(stderr, "seq_dropin: short write to out.bin\n");
    std::exit(2);
  }
  g_out_samples += n;
}

// whether the calling thread's last lora_modulate went through the runtime's queue: only
// that path stamps the modulation's four phases (lora_phy_dropin_last_timing, out[4..7])
bool mod_timing_changed(const double* before) {
  double after[8];
  lora_phy_dropin_last_timing(after);
  return std::memcmp(before + 4, after + 4, 4 * sizeof(double)) != 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: seq_dropin <script.txt> <data.bin> <out.bin>\n");
    return 1;
  }
  std::FILE* fs = std::fopen(argv[1], "r");
  std::FILE* fd = std::fopen(argv[2], "rb");
  g_out = std::fopen(argv[3], "wb");
  if (!fs || !fd || !g_out) {
    std::fprintf(stderr, "seq_dropin: cannot open the script, the data or the output file\n");
    return 2;
  }
  std::fseek(fd, 0, SEEK_END);
  const long dn = std::ftell(fd);
  std::fseek(fd, 0, SEEK_SET);
  g_data.resize(dn > 0 ? (size_t)dn : 0);
  if (!g_data.empty() && std::fread(g_data.data(), 1, g_data.size(), fd) != g_data.size()) return 2;
  std::fclose(fd);
  std::setvbuf(stdout, nullptr, _IOLBF, 0);

  std::vector<Legacy> legacy(kLegacy);
  std::vector<Api> api(kApi);
  auto lw = [&](long w) -> Legacy& {
    if (w < 0 || w >= kLegacy) {
      std::fprintf(stderr, "seq_dropin: legacy workspace %ld\n", w);
      std::exit(2);
    }
    return legacy[(size_t)w];
  };
  auto aw = [&](long w) -> Api& {
    if (w < 0 || w >= kApi) {
      std::fprintf(stderr, "seq_dropin: workspace %ld\n", w);
      std::exit(2);
    }
    return api[(size_t)w];
  };

  char line[512];
  int op = 0;
  while (std::fgets(line, sizeof(line), fs)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind) || kind[0] == '#') continue;
    std::printf("{\"op\": %d, \"kind\": \"%s\"", op, kind.c_str());
    if (kind == "linit") {
      long w;
      unsigned sf, win;
      size_t max_samples;
      std::string scratch;
      if (!(in >> w >> sf >> win >> max_samples >> scratch)) return 2;
      Legacy& L = lw(w);
      cf* sp = nullptr;
      if (scratch != "null") {
        // a fresh buffer first: the workspace may still name the old one until init overwrites it
        std::vector<cf> fresh(max_samples ? max_samples : 1);
        L.scratch.swap(fresh);
        sp = L.scratch.data();
      }
      lora_demod_init(&L.ws, sf, win ? window_type::window_hann : window_type::window_none, sp, max_samples);
      std::printf(", \"N\": %zu", L.ws.N);
      print_state(&L.ws.gpu);
    } else if (kind == "lfree") {
      long w;
      if (!(in >> w)) return 2;
      lora_demod_free(&lw(w).ws);
      print_state(&lw(w).ws.gpu);
    } else if (kind == "ldemod") {
      long w;
      unsigned osr;
      size_t off, n;
      if (!(in >> w >> osr >> off >> n) || osr == 0) return 2;
      Legacy& L = lw(w);
      if (L.ws.N == 0) return 2;
      const cf* x = iq_at(off, n);
      std::vector<uint16_t> out(n / (L.ws.N * osr) + 2, kSymFill);
      uint8_t sync = kSyncFill;
      L.ws.metrics.cfo = kCfoFill;
      L.ws.metrics.time_offset = kToffFill;
      const size_t ret = lora_demodulate(&L.ws, x, n, out.data(), osr, &sync);
      std::printf(", \"ret\": %zu, \"sync\": %u, \"cfo_bits\": %u, \"toff_bits\": %u", ret, sync,
                  fbits(L.ws.metrics.cfo), fbits(L.ws.metrics.time_offset));
      print_symbols(out);
      print_state(&L.ws.gpu);
    } else if (kind == "lmod") {
      unsigned sf, osr, bw, amp_bits, sync;
      size_t off, n;
      if (!(in >> sf >> osr >> bw >> amp_bits >> sync >> off >> n) || sf > 12 || osr == 0) return 2;
      float amp;
      std::memcpy(&amp, &amp_bits, 4);
      const uint16_t* s = syms_at(off, n);
      std::vector<cf> iq((n + 2) * (size_t(1) << sf) * osr);
      double before[8];
      lora_phy_dropin_last_timing(before);
      const size_t ret = lora_modulate(s, n, iq.data(), sf, osr, static_cast<bandwidth>(bw), amp, (uint8_t)sync);
      std::printf(", \"ret\": %zu, \"queue\": %s", ret, mod_timing_changed(before) ? "true" : "false");
      append_out(iq.data(), ret <= iq.size() ? ret : 0);
      print_state(nullptr);
    } else if (kind == "init") {
      long w;
      unsigned sf, osr, bw, win, wbuf, sync;
      if (!(in >> w >> sf >> osr >> bw >> win >> wbuf >> sync) || sf > 12) return 2;
      Api& A = aw(w);
      if (!A.ws) A.ws.reset(new lora_workspace());
      const size_t N = size_t(1) << sf;
      A.symbol_buf.assign(64, 0);
      A.fft_in.assign(N, cf{});
      A.fft_out.assign(N * (osr ? osr : 1), cf{});
      A.window.assign(N, -1.0f);
      A.ws->symbol_buf = A.symbol_buf.data();
      A.ws->fft_in = A.fft_in.data();
      A.ws->fft_out = A.fft_out.data();
      A.ws->window = wbuf ? A.window.data() : nullptr;
      lora_params p{};
      p.sf = sf;
      p.osr = osr;
      p.bw = static_cast<bandwidth>(bw);
      p.window = win ? window_type::window_hann : window_type::window_none;
      p.sync_word = (uint8_t)sync;
      const int ret = init(A.ws.get(), &p);
      const lora_metrics* m = get_last_metrics(A.ws.get());
      // window0: 0 for Hann, 1 for none, the fill above when init was given no window buffer
      std::printf(", \"ret\": %d, \"sync\": %u, \"cfo_bits\": %u, \"toff_bits\": %u, \"window0\": %u", ret,
                  A.ws->sync_word, fbits(m->cfo), fbits(m->time_offset), fbits(A.window[0]));
      print_state(&A.ws->gpu);
    } else if (kind == "demod") {
      long w;
      size_t off, n, cap;
      if (!(in >> w >> off >> n >> cap)) return 2;
      Api& A = aw(w);
      if (!A.ws) return 2;
      const cf* x = iq_at(off, n);
      const size_t step = (size_t(1) << A.ws->gpu.sf) * (A.ws->osr ? A.ws->osr : 1u);
      std::vector<uint16_t> out(std::max(cap, n / step) + 2, kSymFill);
      A.ws->metrics.cfo = kCfoFill;
      A.ws->metrics.time_offset = kToffFill;
      const ssize_t ret = demodulate(A.ws.get(), x, n, out.data(), cap);
      const lora_metrics* m = get_last_metrics(A.ws.get());
      std::printf(", \"ret\": %zd, \"sync\": %u, \"cfo_bits\": %u, \"toff_bits\": %u", ret, A.ws->sync_word,
                  fbits(m->cfo), fbits(m->time_offset));
      print_symbols(out);
      print_state(&A.ws->gpu);
    } else if (kind == "est") {
      long w;
      size_t off, n;
      if (!(in >> w >> off >> n)) return 2;
      Api& A = aw(w);
      if (!A.ws) return 2;
      estimate_offsets(A.ws.get(), iq_at(off, n), n);
      const lora_metrics* m = get_last_metrics(A.ws.get());
      std::printf(", \"sync\": %u, \"cfo_bits\": %u, \"toff_bits\": %u", A.ws->sync_word, fbits(m->cfo),
                  fbits(m->time_offset));
      print_state(&A.ws->gpu);
    } else if (kind == "comp") {
      long w;
      size_t off, n;
      if (!(in >> w >> off >> n)) return 2;
      Api& A = aw(w);
      if (!A.ws) return 2;
      const cf* x = iq_at(off, n);
      std::vector<cf> io(x, x + n);
      compensate_offsets(A.ws.get(), io.data(), n);
      const lora_metrics* m = get_last_metrics(A.ws.get());
      std::printf(", \"sync\": %u, \"cfo_bits\": %u, \"toff_bits\": %u", A.ws->sync_word, fbits(m->cfo),
                  fbits(m->time_offset));
      append_out(io.data(), n);
      print_state(&A.ws->gpu);
    } else if (kind == "mod") {
      long w;
      size_t off, n, cap;
      if (!(in >> w >> off >> n >> cap)) return 2;
      Api& A = aw(w);
      if (!A.ws) return 2;
      const uint16_t* s = syms_at(off, n);
      const size_t need = (n + 2) * (size_t(1) << A.ws->gpu.sf) * (A.ws->osr ? A.ws->osr : 1u);
      std::vector<cf> iq(std::max(need, cap));
      const ssize_t ret = modulate(A.ws.get(), s, n, iq.data(), cap);
      std::printf(", \"ret\": %zd", ret);
      append_out(iq.data(), ret > 0 && (size_t)ret <= iq.size() ? (size_t)ret : 0);
      print_state(&A.ws->gpu);
    } else if (kind == "destroy") {
      long w;
      if (!(in >> w)) return 2;
      aw(w).ws.reset();
      print_state(nullptr);
    } else {
      std::fprintf(stderr, "seq_dropin: unknown operation '%s'\n", kind.c_str());
      return 2;
    }
    ++op;
  }
  std::fclose(fs);
  // every workspace is released while the HIP runtime is alive (lora_mi355x_phy.hpp)
  for (Api& A : api) A.ws.reset();
  for (Legacy& L : legacy) lora_demod_free(&L.ws);
  std::fclose(g_out);
  std::printf("{\"ops\": %d, \"dropin_status\": %d}\n", op, lora_phy_dropin_status());
  return 0;
}
