// Tests of the trace preflight through the C++ host mirror (include/zkl_hip.hpp: PreflightMode,
// PreflightReport, ZkProver::check, Device::set_preflight_mode, eval_transition_row), written the
// way the reference's callers use preflight::run / with_preflight_mode (prove.rs:188-212).
//   preflight_api_test cpu   the host-only resolution step and the report's text, no device
//   preflight_api_test gpu   checks a valid and a corrupted 2^10-row segment on device 0, alone and
//                            as the opt-in step in front of prove
// Prints "ok ..." and exits 0 on success; any failure exits 1 with the reason.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "zkl_hip.hpp"

namespace {

int g_fail = 0;
#define EXPECT(c)                                                        \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail = 1;                                                        \
    }                                                                    \
  } while (0)

struct Segment {
  zkl::TraceTable trace;
  zkl::AirPublicInputs pi;
};
Segment synth_segment(uint64_t seed, uint32_t log_n) {
  uint32_t w = 0;
  zkl::detail::check(zkl_synth_vm_segment(seed, log_n, nullptr, nullptr, &w));
  Segment s{zkl::TraceTable(w, 1u << log_n), zkl::AirPublicInputs()};
  zkl::detail::check(zkl_synth_vm_segment(seed, log_n, s.trace.data(), &s.pi, &w));
  return s;
}

std::vector<zkl::BaseElement> row_of(const zkl::TraceTable& t, uint32_t r) {
  std::vector<zkl::BaseElement> v(t.width());
  for (uint32_t c = 0; c < t.width(); c++) v[c] = t.get(c, r);
  return v;
}

// first non-zero constraint of rows (r, r + 1), or -1
int first_violation(const Segment& s, uint32_t r, zkl::BaseElement* value = nullptr) {
  const auto vals = zkl::eval_transition_row(s.trace.width(), s.trace.length(), s.pi, r, row_of(s.trace, r).data(),
                                             row_of(s.trace, r + 1).data());
  for (size_t i = 0; i < vals.size(); i++)
    if (vals[i].lo | vals[i].hi) {
      if (value) *value = vals[i];
      return (int)i;
    }
  return -1;
}

template <class F>
std::string backend_message(F&& f) {
  try {
    f();
  } catch (const zkl::Error& e) {
    return e.kind() == zkl::Error::Kind::Backend && e.code() == ZKL_E_INVALID ? e.what() : "";
  }
  return "";
}

// register r3 (column 45 of the {vm, rom} layout) at row 300: the write-back constraint of r3 at
// row 299 is the first to fail
void corrupt(Segment& s) {
  zkl::BaseElement v = s.trace.get(45, 300);
  v.lo ^= 1;
  s.trace.set(45, 300, v);
}

int run_cpu() {
  Segment s = synth_segment(0x5EED0001, 10);
  const uint32_t w = s.trace.width(), n = s.trace.length();
  EXPECT(w == 204 && n == 1024);
  const auto vals = zkl::eval_transition_row(w, n, s.pi, 0, row_of(s.trace, 0).data(), row_of(s.trace, 1).data());
  EXPECT(vals.size() == 193);  // Ctrl 91 + ALU 16 + ROM 86
  for (uint32_t r : {0u, 298u, 299u, 300u, n - 2}) EXPECT(first_violation(s, r) == -1);
  corrupt(s);
  zkl::BaseElement v{};
  EXPECT(first_violation(s, 298) == -1);
  EXPECT(first_violation(s, 299, &v) == 94);
  EXPECT(first_violation(s, 300) >= 0);
  // the last row has no transition; a wrong width is the request's error
  EXPECT(backend_message([&] {
           (void)zkl::eval_transition_row(w, n, s.pi, n - 1, row_of(s.trace, n - 1).data(), row_of(s.trace, n - 1).data());
         }).find("last row") != std::string::npos);
  EXPECT(!backend_message([&] {
            (void)zkl::eval_transition_row(w - 1, n, s.pi, 0, row_of(s.trace, 0).data(), row_of(s.trace, 1).data());
          }).empty());
  // the report's console line and JSON field names (preflight.rs:29-70)
  zkl::PreflightReport rep;
  rep.kind = 1;
  rep.index = 94;
  rep.row = 299;
  rep.pos = 299 % 32;
  rep.value = v;
  EXPECT(rep.to_string() == "preflight: constraint 94 non-zero at row 299: " + zkl::detail::fe_decimal(v));
  const std::string js = rep.to_json();
  for (const char* k : {"\"row\":299", "\"constraint_idx\":94", "\"constraint_val\":", "\"pos\":11", "\"gates_map\":",
                        "\"gates_final\":", "\"rounds\":[", "\"lanes_cur\":[", "\"lanes_next\":[", "\"lanes_exp\":null",
                        "\"ram\":null", "\"vm\":null", "\"peak_live\":null"})
    EXPECT(js.find(k) != std::string::npos);
  EXPECT(zkl::detail::fe_decimal(zkl::BaseElement{0, 1}) == "18446744073709551616");
  if (g_fail) return 1;
  std::printf("ok cpu\n");
  return 0;
}

int run_gpu() {
  Segment good = synth_segment(0x5EED0001, 10), bad = synth_segment(0x5EED0001, 10);
  corrupt(bad);
  const uint32_t w = good.trace.width(), n = good.trace.length();
  const zkl::ProofOptions opts = zkl::ProofOptions(32, 16, 8).for_trace(w, n);
  zkl::Device dev(0);
  EXPECT(dev.preflight_mode() == zkl::PreflightMode::Off);
  const zkl::ZkProver prover(opts, good.pi, dev);
  EXPECT(!prover.check(good.trace).has_value());
  EXPECT(!prover.check(good.trace, 7).has_value());
  const auto rep = prover.check(bad.trace);
  zkl::BaseElement v{};
  EXPECT(first_violation(bad, 299, &v) == 94);
  EXPECT(rep.has_value() && rep->is_transition() && rep->row == 299 && rep->index == 94 && rep->pos == 299 % 32);
  EXPECT(rep.has_value() && rep->value.lo == v.lo && rep->value.hi == v.hi);
  // off: the prover's own refusal; on: the preflight's, and the report stays on the Device
  EXPECT(backend_message([&] { (void)prover.prove(bad.trace); }).find("degree too large") != std::string::npos);
  const zkl::Proof proof = prover.prove(good.trace);
  dev.set_preflight_mode(zkl::PreflightMode::On);
  EXPECT(dev.preflight_mode() == zkl::PreflightMode::On);
  EXPECT(backend_message([&] { (void)prover.prove(bad.trace); })
             .find("preflight: constraint 94 non-zero at row 299: " + zkl::detail::fe_decimal(v)) != std::string::npos);
  const auto last = dev.last_report();
  EXPECT(last.has_value() && last->row == 299 && last->index == 94);
  EXPECT(prover.prove(good.trace).bytes == proof.bytes);
  EXPECT(!dev.last_report().has_value());
  dev.set_preflight_mode(zkl::PreflightMode::Off);
  // a changed public input: the first failing assertion (pc at row 0)
  Segment as = synth_segment(0x5EED0001, 10);
  as.pi.pc_init.lo += 1;
  const auto arep = zkl::ZkProver(opts, as.pi, dev).check(as.trace);
  EXPECT(arep.has_value() && arep->is_assertion() && arep->row == 0 && arep->expected.lo == as.pi.pc_init.lo);
  EXPECT(arep.has_value() && arep->value.lo == as.trace.get(arep->column, 0).lo);
  if (g_fail) return 1;
  std::printf("ok gpu preflight: %s\n", rep->to_string().c_str());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "cpu";
  try {
    if (mode == "cpu") return run_cpu();
    if (mode == "gpu") return run_gpu();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  std::fprintf(stderr, "usage: preflight_api_test cpu | gpu\n");
  return 2;
}
