// host_selftest.cpp -- CPU-only checks of the host mirror's small pieces against the behaviour
// the reference documents (file:line cited per block).  Run by tests/test_host.py.
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sys/wait.h>
#include <unistd.h>
#include <iostream>
#include <sstream>
#include <type_traits>

#include "arithexpr_evaluator.h"
#include "csv_utils.h"
#include "kernel_config.h"
#include "kernel_utils.h"
#include "run.h"
#include "sparse_matrix.h"
#include "spmv_gold.h"
#include "sql_stat.h"
#include "vector_generator.h"

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

// `host_selftest --encode <matrix.mtx> <kernel.json>...`: load each kernel config and run
// executorEncodeMatrix on the matrix (no GPU involved); one line per config.  tests/test_host.py
// points it at the reference's own example/*/kernel*.json files to show that they are accepted as they are.
template <typename T> static int encode_probe(const std::string &matrix, int n, char **jsons) {
  SparseMatrix<T> m{matrix};
  ConstXVectorGenerator<T> x((T)1);
  ConstYVectorGenerator<T> y((T)0);
  for (int i = 0; i < n; i++) {
    KernelConfig<T> kc{std::string(jsons[i])};
    auto args = executorEncodeMatrix(1ul << 30, kc, m, (T)0, x, y, (T)1, (T)0);
    const std::string &src = kc.getSource();
    const char *sr = std::is_integral<T>::value
                         ? ((src.find("int_max") != std::string::npos || src.find("doubleMinMax") != std::string::npos) ? "max-min" : "or-and")
                         : ((src.find("clmin") != std::string::npos || src.find("absadd") != std::string::npos) ? "min-plus" : "plus-times");
    std::printf("ENCODE %s name=%s semiring=%s rows=%d cols=%d size_args=", jsons[i], kc.getName().c_str(), sr, args.rows, args.cols);
    for (unsigned v : args.size_args) std::printf("%u,", v);
    std::printf(" output=%u temp_globals=%zu temp_locals=%zu x=%zu idxs=%zu\n", args.output, args.temp_globals.size(),
                args.temp_locals.size(), args.x_vect.size(), args.m_idxs.size());
  }
  return 0;
}

// FNV-1a over the bytes of an array: the checksum `--load` prints
template <typename V> static unsigned long long fnv(const std::vector<V> &a) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char *p = reinterpret_cast<const unsigned char *>(a.data());
  for (std::size_t i = 0; i < a.size() * sizeof(V); i++)
    h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

// `host_selftest --load <matrix.mtx> <elem_is_int> <normalise>`: what sh_mm_load_ex does (load, then the PageRank
// (1) or SCC (2) normaliser), then Gold<T>::spmv with x = 1; one line with the dims and a checksum per array.  A
// refused file ends the process inside the loader (exit(-1)).
template <typename T> static int load_probe(const std::string &matrix, int normalise) {
  SparseMatrix<T>::set_truncate(true);
  SparseMatrix<T>::set_keep_entries(normalise == 1);
  SparseMatrix<T> m{matrix};
  SparseMatrix<T>::set_keep_entries(false);
  if (normalise == 1)
    m.pagerank_normalise(0.85f, 0);
  else if (normalise == 2)
    m.scc_normalise();
  // the loader's invariant (inc/sparse_matrix.h), checked before the gold walks the arrays
  const auto &rp = m.rowPtr();
  const auto &ci = m.colIdx();
  bool sound = rp.size() == (std::size_t)m.height() + 1 && rp.front() == 0 && rp.back() == m.storedNonZeros() &&
               m.values().size() == ci.size();
  for (std::size_t r = 0; sound && r + 1 < rp.size(); r++)
    sound = rp[r] <= rp[r + 1];
  for (std::size_t k = 0; sound && k < ci.size(); k++)
    sound = ci[k] >= 0 && ci[k] < m.width();
  if (!sound) {
    std::printf("LOAD %s breaks the loader's invariant\n", matrix.c_str());
    return 1;
  }
  ConstXVectorGenerator<T> x((T)1);
  ConstYVectorGenerator<T> y((T)0);
  auto gold = Gold<T>::spmv(m, x, y, (T)1, (T)0, (T)0);
  std::printf("LOAD rows=%d cols=%d header_nnz=%d nnz=%lld max_row=%u row_ptr=%016llx col_idx=%016llx val=%016llx gold=%016llx\n",
              m.height(), m.width(), m.nonZeros(), (long long)m.storedNonZeros(), m.maxRowLength(), fnv(rp), fnv(ci),
              fnv(m.values()), fnv(gold));
  return 0;
}

// Runs KernelConfig<float>(path) in a forked child, stderr into `log`: true when the child ended as a refused
// kernel file does -- exit(-1) and a "Bad kernel file" line -- and in no other way (abort, signal, success).
static bool refused_as_bad_kernel_file(const std::string &path, const std::string &log) {
  std::fflush(stdout);
  const pid_t pid = fork();
  if (pid == 0) {
    if (!std::freopen(log.c_str(), "w", stderr)) _exit(99);
    KernelConfig<float> kc{path};
    _exit(0);
  }
  int status = 0;
  if (pid < 0 || waitpid(pid, &status, 0) != pid || !WIFEXITED(status) || WEXITSTATUS(status) != 255)
    return false;
  std::stringstream ss;
  ss << std::ifstream(log).rdbuf();
  return ss.str().find("Bad kernel file") != std::string::npos;
}
static bool bad_kernel_text(const std::string &dir, const std::string &text) {
  std::ofstream(dir + "/bad.json", std::ios::binary) << text;
  return refused_as_bad_kernel_file(dir + "/bad.json", dir + "/bad.log");
}

int main(int argc, char **argv) {
  if (argc >= 4 && (std::string(argv[1]) == "--encode" || std::string(argv[1]) == "--encode-int"))
    return std::string(argv[1]) == "--encode" ? encode_probe<float>(argv[2], argc - 3, argv + 3)
                                              : encode_probe<int>(argv[2], argc - 3, argv + 3);
  if (argc == 5 && std::string(argv[1]) == "--load")
    return std::atoi(argv[3]) ? load_probe<int>(argv[2], std::atoi(argv[4])) : load_probe<float>(argv[2], std::atoi(argv[4]));
  // `host_selftest --eval <MWidthC> <MHeight> <VLength> <expr>...`: one evaluated size per line
  if (argc >= 5 && std::string(argv[1]) == "--eval") {
    for (int i = 5; i < argc; i++)
      std::printf("%d\n", Evaluator::evaluate(argv[i], std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])));
    return 0;
  }
  // `host_selftest --runs <runfile>`: read a run file as the apps do
  if (argc == 3 && std::string(argv[1]) == "--runs") {
    for (auto &l : CSV::load_csv(argv[2]))
      std::cout << "RUN " << Run(l) << "\n";
    return 0;
  }
  const std::string dir = argc > 1 ? argv[1] : ".";
  // ---- a run-file line that is not six numbers is told apart, not asserted on (inc/run.h)
  {
    Run r(0, 0, 0, 0, 0, 0);
    std::string why;
    CHECK(Run::parse(CSV::tokenise_line("1280,1,1,128,1,1,"), r, why) && r.global1 == 1280 && r.local1 == 128);
    CHECK(Run::parse(CSV::tokenise_line(" 7 ,1,1,128,1,1\r"), r, why) && r.global1 == 7 && r.local3 == 1);
    CHECK(!Run::parse(CSV::tokenise_line("1280,1,1,128,1"), r, why) && why.find("found 5") != std::string::npos);
    CHECK(!Run::parse(CSV::tokenise_line("1280,1,1,128,1,1,1"), r, why));
    CHECK(!Run::parse(CSV::tokenise_line("1280,1,x,128,1,1"), r, why) && why.find("field 3") != std::string::npos);
    CHECK(!Run::parse(CSV::tokenise_line("1280,1,-1,128,1,1"), r, why));
    CHECK(!Run::parse(CSV::tokenise_line("1280,1,,128,1,1"), r, why));
    CHECK(!Run::parse(CSV::tokenise_line("1280,1,1.5,128,1,1"), r, why));
    CHECK(!Run::parse(CSV::tokenise_line("99999999999999999999,1,1,128,1,1"), r, why));
  }
  // ---- kernel files that must be refused as "Bad kernel file" with exit(-1), never an abort (src/kernel_config.cpp)
  {
    const std::string head = R"J({"name":"n","source":"s",)J";
    const std::string props = R"J("properties":{"chunkSize":128},)J";
    const std::string tail = R"J("inputArgs":[],"outputArg":{"variable":"o","addressSpace":"global","size":"4"},)J"
                             R"J("tempGlobals":[],"tempLocals":[],"paramVars":[]})J";
    std::ofstream(dir + "/good.json") << head + props + tail;
    CHECK(!refused_as_bad_kernel_file(dir + "/good.json", dir + "/good.log"));    // the pieces are a good file
    CHECK(bad_kernel_text(dir, R"J({"name":"\u12zz","source":"s",)J" + props + tail));   // \u with non-hex digits
    CHECK(bad_kernel_text(dir, R"J({"name":"\u00)J"));
    CHECK(bad_kernel_text(dir, R"J({"name":"n","source":"never closed)J"));     // unterminated string
    CHECK(bad_kernel_text(dir, head + tail));                                     // no `properties`
    CHECK(bad_kernel_text(dir, head + R"J("properties":{"chunkSize":"abc"},)J" + tail));
    CHECK(bad_kernel_text(dir, std::string(100000, '[')));                        // nesting limit (inc/mini_json.h)
    CHECK(bad_kernel_text(dir, std::string(100000, '{')));
    std::string deep = head + props + "\"unknownKey\":" + std::string(64, '[') + std::string(64, ']') + "," + tail.substr(0);
    CHECK(bad_kernel_text(dir, deep));                                            // 1 + 64 levels: one too many
    deep = head + props + "\"unknownKey\":" + std::string(63, '[') + std::string(63, ']') + "," + tail;
    std::ofstream(dir + "/deep.json") << deep;
    CHECK(!refused_as_bad_kernel_file(dir + "/deep.json", dir + "/deep.log"));    // 64 levels are read
    // every proper prefix of a shipped kernel file (argv[2]), one child each
    if (argc > 2) {
      std::stringstream ss;
      ss << std::ifstream(argv[2]).rdbuf();
      std::string whole = ss.str();
      while (!whole.empty() && std::isspace((unsigned char)whole.back())) whole.pop_back();
      CHECK(whole.size() > 100);
      std::size_t accepted = 0;
      for (std::size_t n = 0; n < whole.size(); n++)
        accepted += !bad_kernel_text(dir, whole.substr(0, n));
      if (accepted) std::printf("FAIL %zu of %zu prefixes of %s were not refused as a bad kernel file\n", accepted, whole.size(), argv[2]);
      failures += accepted != 0;
      std::printf("kernel file prefixes refused: %zu of %zu\n", whole.size() - accepted, whole.size());
    }
  }
  // ---- run-file: 6 fields, trailing comma tolerated, stop at first blank line (inc/csv_utils.h:16-49, src/run.cpp:4-16)
  {
    std::ofstream(dir + "/runs.csv") << "1280,1,1,128,1,1,\n524288,1,1,256,1,1\n\n99,9,9,9,9,9\n";
    auto lines = CSV::load_csv(dir + "/runs.csv");
    CHECK(lines.size() == 2);
    Run r0(lines[0]), r1(lines[1]);
    CHECK(r0.global1 == 1280 && r0.local1 == 128 && r0.num_work_items() == 128);
    CHECK(r1.global1 == 524288 && r1.local1 == 256 && r1.global3 == 1);
    std::ostringstream os;
    os << r0;
    CHECK(os.str() == "{1280 1 1 / 128 1 1}");
  }
  // ---- size expressions of the kernel JSON (src/arithexpr_evaluator.cpp:10-30)
  CHECK(Evaluator::evaluate("(4*v_MHeight_2*v_MWidthC_1)", 18, 1138, 1138) == 4 * 1138 * 18);
  CHECK(Evaluator::evaluate("(4*v_VLength_3)", 1, 2, 300) == 1200);
  CHECK(Evaluator::evaluate("4", 1, 2, 3) == 4);
  CHECK(Evaluator::evaluate("(8+(4*v_MWidthC_1))/2", 6, 0, 0) == 16);
  CHECK(Evaluator::evaluate("?", 1, 2, 3) == 0);          // quirk A-13: non-numeric sizes
  CHECK(Evaluator::evaluate("(4*v_Unknown)", 1, 2, 3) == 0);
  // ---- SQL row text, byte for byte (inc/sql_stat.h:28-79)
  {
    std::vector<SqlStat> st{SqlStat(std::chrono::nanoseconds(1500000), CORRECT, 1280, 128, RAW_RESULT, 2, 3),
                            SqlStat(std::chrono::nanoseconds(250), STATISTIC_VALUE, 1280, 128, MEDIAN_RESULT)};
    const std::string sql = SqlStat::makeSqlCommand(st, "k", "h", "d", "m", "e");
    CHECK(sql == "INSERT INTO table_name (time, correct, kernel, global, local, host, device, matrix, iteration, "
                 "trial,statistic, experiment_id) VALUES (1.5, \"correct\", \"k\", 1280, 128, \"h\", \"d\", \"m\",3,2,"
                 "\"RAW_RESULT\", \"e\"), (0.00025, \"statisticvalue\", \"k\", 1280, 128, \"h\", \"d\", \"m\",0,0,"
                 "\"MEDIAN_RESULT\", \"e\");");
    CHECK(SqlStat::compare(st[1], st[0]) && !SqlStat::compare(st[0], st[1]));
  }
  // ---- kernel config JSON: optional properties default to "nothing"/-1, numbers-as-strings (src/kernel_config.cpp:8-96)
  {
    std::ofstream(dir + "/k.json") << R"JSON({"name":"awrg-alcl-alcl-edp-split-8","source":"float clmin(float a,float b){}\n\"quoted\" \\ A",
      "properties":{"splitSize":"8","innerMap":"alcl","outerMap":"awrg","chunkSize":128,"dotProduct":"earlyexit","extra":true},
      "inputArgs":[{"variable":"v1","addressSpace":"global","size":"?"}],
      "tempGlobals":[{"variable":"t","addressSpace":"global","size":"4"}],
      "outputArg":{"variable":"o","addressSpace":"global","size":"(4*v_MHeight_2)"},
      "tempLocals":[{"variable":"l","addressSpace":"local","size":"(4*v_MWidthC_1)"}],
      "paramVars":["MHeight","MWidthC","VLength"],"outputSize":"(4*v_MHeight_2)","unknownKey":[1,2,{"a":null}]})JSON";
    KernelConfig<float> kc(dir + "/k.json");
    auto p = kc.getProperties();
    CHECK(kc.getName() == "awrg-alcl-alcl-edp-split-8");
    CHECK(p.splitSize == 8 && p.chunkSize == 128 && p.outerMap == "awrg" && p.innerMap2 == "nothing" && p.arrayType == "nothing");
    CHECK(kc.getSource().find("clmin") != std::string::npos && kc.getSource().find("\"quoted\" \\ A") != std::string::npos);
    CHECK(kc.getTempLocals().size() == 1 && kc.getParamVars().size() == 3 && kc.getOutputArg()->size == "(4*v_MHeight_2)");
    CHECK(kc.getArgs()[0].size == "?");
  }
  // ---- loader + encode + gold on a tiny symmetric file, incl. quirks A-1, A-3, A-6
  {
    std::ofstream(dir + "/m.mtx") << "%%MatrixMarket matrix coordinate real symmetric\n% c\n3 3 3\n1 1 2.9\n3 1 -1.5\n2 3 4\n";
    SparseMatrix<float> m(dir + "/m.mtx");
    CHECK(m.height() == 3 && m.width() == 3 && m.nonZeros() == 3 && m.storedNonZeros() == 5);
    // row = file column: row0 = {(0,2),(2,-1)}, row1 = {(2,4)}, row2 = {(0,-1),(1,4)} with values narrowed through int
    CHECK(m.rowPtr() == (std::vector<int32_t>{0, 2, 3, 5}));
    CHECK(m.colIdx() == (std::vector<int32_t>{0, 2, 2, 0, 1}));
    CHECK(m.values() == (std::vector<float>{2.f, -1.f, 4.f, -1.f, 4.f}));
    ConstXVectorGenerator<float> x(1.0f);
    ConstYVectorGenerator<float> y(0.0f);
    auto gold = Gold<float>::spmv(m, x, y, 1.0f, 0.0f, 0.0f);
    CHECK(gold == (std::vector<float>{1.f, 4.f, 3.f}));
    KernelConfig<float> kc(dir + "/k.json");   // chunkSize 128 -> height 3 + (128 - 3 % 128) = 128
    auto args = executorEncodeMatrix(1ul << 30, kc, m, 0.0f, x, y, 1.0f, 0.0f);
    CHECK(args.rows == 128 && args.cols == 128 && args.output == 4 * 128);
    CHECK(args.x_vect.size() == 4 * 128 && args.m_row_ptr.size() == 4 * 129 && args.m_idxs.size() == 4 * 5);
    CHECK(args.size_args == (std::vector<unsigned>{128, 1, 128}));   // MHeight, MWidthC = (2 + (8 - 2 % 8)) / 8, VLength
    CHECK(args.temp_globals == (std::vector<unsigned>{4}) && args.temp_locals == (std::vector<unsigned>{4}));
    bool threw = false;
    try { (void)executorEncodeMatrix(8ul, kc, m, 0.0f, x, y); } catch (unsigned long n) { threw = n == 20; }
    CHECK(threw);                                                    // oversize -> throw unsigned long (src/sparse_matrix.cpp:231-233)
  }
  std::printf(failures ? "host selftest: %d FAILED\n" : "host selftest: all passed\n", failures);
  return failures ? 1 : 0;
}
