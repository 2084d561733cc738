// model_asan_main.cpp — the model-step entries of tests/prims/model_entries.h as a stand-alone program for the
// AddressSanitizer + UBSan run of the CPU tier (TEST INFRASTRUCTURE ONLY; tests/emul_model_asan.py builds and runs it).
//
//   model_asan_main IN OUT
// IN : int64 kind, B, p, nF, seed; double reg_rel; then H [B * h] doubles (the entry's layout), theta [B * p], g [B * p]
//      doubles, ord [B * p] uint16.
// OUT: int32 rc; then tc [B * p] doubles, moved [B] int32, sact [B * nI] bytes, ss [B * nI] doubles, M [B * m] doubles.
// Every buffer is a heap block of its exact size, and the workgroup's LDS is one too (simt_abi.cpp Lds): a read or write
// past any of them stops the program.  Prints "model-asan-ok".
#include "simt_abi.cpp"

#include <cstdio>

namespace {

template <class T>
std::vector<T> read_n(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
template <class T>
void write_n(FILE* f, const std::vector<T>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short output\n"); exit(2); }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  const std::vector<int64_t> hd = read_n<int64_t>(in, 5);
  const double reg_rel = read_n<double>(in, 1)[0];
  const int32_t kind = (int32_t)hd[0], p = (int32_t)hd[2], nF = (int32_t)hd[3];
  const int64_t B = hd[1];
  const uint64_t seed = (uint64_t)hd[4];
  const int64_t h = cave_simt_prim_info(kind, 0, p, nF, 0);
  if (h < 0 || B < 0 || B > 64 || kind < cave_prims::K_LITE_MODEL) return 3;
  const size_t nI = (size_t)(p - nF), m = kind == cave_prims::K_LITE_MODEL ? (size_t)p * (size_t)(p | 1) : 1;
  const std::vector<double> H = read_n<double>(in, (size_t)(B * h));
  const std::vector<double> theta = read_n<double>(in, (size_t)B * p), g = read_n<double>(in, (size_t)B * p);
  const std::vector<uint16_t> ord = read_n<uint16_t>(in, (size_t)B * p);
  fclose(in);
  const double poison = cave_prims::poison_f64();
  std::vector<double> tc((size_t)B * p, poison), ss((size_t)B * nI, poison), M((size_t)B * m, poison);
  std::vector<int32_t> moved((size_t)B, -7);
  std::vector<uint8_t> sact((size_t)B * nI, 0xee);
  cave_prims::PrimBatch a{};
  a.B = B; a.p = p; a.nF = nF; a.reg_rel = reg_rel;
  a.H = H.data(); a.h_stride = h; a.M = M.data(); a.m_stride = (int64_t)m;
  a.theta = theta.data(); a.g = g.data(); a.ord = ord.data();
  a.tc = tc.data(); a.moved = moved.data(); a.sact_out = sact.data(); a.ss_out = ss.data();
  const int32_t rc = cave_simt_prim_run(kind, &a, seed);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  write_n(out, std::vector<int32_t>{rc});
  write_n(out, tc); write_n(out, moved); write_n(out, sact); write_n(out, ss); write_n(out, M);
  fclose(out);
  printf("model-asan-ok\n");
  return 0;
}
