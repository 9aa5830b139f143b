// bvcf_bgzf_out.cpp — the compressed output stream of bvcf_run_fd (bvcf_config.out_bgzf): see bvcf_bgzf_out.h.
//
// The stream is cut every kPiece bytes of the OUTPUT, whatever the batches, devices or input kind were, so the file
// depends on the TSV bytes only.  The caller (the header line, then the ordered sink) fills a pinned staging buffer of
// kBufPieces whole pieces; a full one is handed to the compressor thread, which runs k_deflate and the rest on its own
// stream of the run's first device and writes the members to fd in order.  kBufs buffers: one being filled, the others
// on the device or being written.
#include "bvcf_bgzf_out.h"

#include "../../include/bvcf.h"
#include "bvcf_host_internal.h"

#include <string.h>

namespace bvcf_bgzf_out {

namespace {
constexpr size_t kBufPieces = 257;  // 16.8 MB of text per buffer
constexpr int kBufs = 3;
}  // namespace

BgzfWriter::~BgzfWriter() {
  if (th_.joinable()) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    th_.join();
  }
  for (Buf &b : bufs_) {
    bvcf_free_pinned(b.text);
    bvcf_free_pinned(b.out);
  }
  deflate_close(run_);
}

int BgzfWriter::open(std::string *err) {
  buf_bytes_ = kBufPieces * kPiece;
  run_ = deflate_open(device_, buf_bytes_, err);
  if (!run_) return -1;
  for (int i = 0; i < kBufs; i++) {
    Buf b;
    b.text = (uint8_t *)bvcf_alloc_pinned_near(device_, buf_bytes_);
    b.out = (uint8_t *)bvcf_alloc_pinned_near(device_, bound(buf_bytes_));
    bufs_.push_back(b);
    if (!b.text || !b.out) {
      *err = "pinned staging buffers of the compressed output";
      return -1;
    }
    free_.push_back(i);
  }
  cur_ = free_.front();
  free_.pop_front();
  th_ = std::thread([this] { loop(); });
  return 0;
}

void BgzfWriter::loop() {
  for (;;) {
    int i;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return stop_ || !full_.empty(); });
      if (full_.empty()) return;
      i = full_.front();
      full_.pop_front();
    }
    Buf &b = bufs_[i];
    const double t0 = bvcf_host::now_s();
    if (!failed_.load()) {
      size_t n_out = 0;
      double ms = 0;
      std::string e;
      const int rc = deflate_run(run_, b.text, b.n, b.out, bound(buf_bytes_), &n_out, &ms, &e);
      if (rc != BVCF_OK) {
        err_ = "compressed output: " + e;
        failed_.store(true);
      } else if (bvcf_host::write_all(fd_, (const char *)b.out, n_out)) {
        err_ = "write failed";
        failed_.store(true);
      } else {
        text_bytes += b.n;
        out_bytes += n_out;
        kernel_ms += ms;
        buffers++;
      }
    }
    busy_s += bvcf_host::now_s() - t0;
    b.n = 0;
    {
      std::lock_guard<std::mutex> lk(mu_);
      free_.push_back(i);
    }
    cv_.notify_all();
  }
}

int BgzfWriter::write(const char *p, size_t n) {
  while (n) {
    if (failed_.load()) return -1;
    Buf &b = bufs_[cur_];
    const size_t k = std::min(n, buf_bytes_ - b.n);
    memcpy(b.text + b.n, p, k);
    b.n += k;
    p += k;
    n -= k;
    if (b.n == buf_bytes_) {
      const double t0 = bvcf_host::now_s();
      std::unique_lock<std::mutex> lk(mu_);
      full_.push_back(cur_);
      cv_.notify_all();
      cv_.wait(lk, [&] { return !free_.empty(); });
      cur_ = free_.front();
      free_.pop_front();
      wait_s += bvcf_host::now_s() - t0;
    }
  }
  return failed_.load() ? -1 : 0;
}

int BgzfWriter::finish(bool add_eof) {
  {
    std::lock_guard<std::mutex> lk(mu_);
    if (bufs_[cur_].n) full_.push_back(cur_);
    stop_ = true;
  }
  cv_.notify_all();
  th_.join();
  if (failed_.load()) return -1;
  if (add_eof) {
    if (bvcf_host::write_all(fd_, (const char *)kEofBlock, sizeof kEofBlock)) {
      err_ = "write failed";
      failed_.store(true);
      return -1;
    }
    out_bytes += sizeof kEofBlock;
  }
  return 0;
}

}  // namespace bvcf_bgzf_out
