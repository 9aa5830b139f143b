#pragma once
// bvcf_bgzf_out.h — BGZF output compressed on the device (bvcf_config.out_bgzf, bvcf_bgzf_deflate_device).
// DeflateRun: the device half (bvcf_core.hip; kernels in bvcf_deflate.hip.h).  BgzfWriter: the ordered byte stream of a run
// cut every 65 280 bytes into BGZF members, several staging buffers in flight (bvcf_bgzf_out.cpp).
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace bvcf_bgzf_out {

constexpr size_t kPiece = 65280;  // text per member (bgzip's cut)
constexpr size_t kMemberMax = 65311;  // 18 + 5 + kPiece + 8: one stored member
extern const uint8_t kEofBlock[28];  // the standard empty end-of-file member

inline size_t bound(size_t n) { return (n + kPiece - 1) / kPiece * kMemberMax + 28; }

// the device buffers and the stream of one compressor; text of up to max_text bytes per call
struct DeflateRun;
DeflateRun *deflate_open(int device, size_t max_text, std::string *err);
// text[0, n) (host memory) -> BGZF members at out (host), cut every kPiece bytes; synchronous on the run's stream.
// BVCF_E_TOO_BIG if cap is short (*n_out: the bytes needed).  *kernel_ms: the kernels' time (events).
int deflate_run(DeflateRun *r, const uint8_t *text, size_t n, uint8_t *out, size_t cap, size_t *n_out, double *kernel_ms,
                std::string *err);
void deflate_close(DeflateRun *r);

// write() appends to a pinned staging buffer of whole pieces; a full buffer goes to the compressor thread, which runs the
// kernels on the device and writes the members to fd in order.  write() waits for a free buffer when all are in
// flight, so a slow compressor holds the caller exactly as a slow fd does.
class BgzfWriter {
 public:
  BgzfWriter(int fd, int device) : fd_(fd), device_(device) {}
  ~BgzfWriter();
  int open(std::string *err);
  int write(const char *p, size_t n);  // 0, or -1 once the compressor or fd_out failed
  // the partial last buffer, then (add_eof) the end-of-file block; waits for everything to be written.  0 or -1
  int finish(bool add_eof);
  bool failed() const { return failed_.load(); }
  const std::string &error() const { return err_; }
  // timing
  uint64_t text_bytes = 0, out_bytes = 0, buffers = 0;
  double kernel_ms = 0, busy_s = 0, wait_s = 0;

 private:
  void loop();
  int fd_, device_;
  size_t buf_bytes_ = 0;
  struct Buf {
    uint8_t *text = nullptr, *out = nullptr;
    size_t n = 0;
  };
  std::vector<Buf> bufs_;
  DeflateRun *run_ = nullptr;
  int cur_ = -1;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<int> full_, free_;
  bool stop_ = false;
  std::atomic<bool> failed_{false};
  std::string err_;
  std::thread th_;
};

}  // namespace bvcf_bgzf_out
