#include "stager.h"

#include <errno.h>
#include <time.h>

#include <chrono>
#include <cstring>
#include <stdexcept>

namespace mrl {

namespace {

// Health checks run every kHealthEvery slices of kSliceMs: a 2 s period, as in
// EnvPool::result(). The slice only bounds how long a stop request waits for a
// thread that is blocked on a worker's semaphore.
constexpr long kSliceMs = 100;
constexpr int kHealthEvery = 20;
constexpr std::chrono::seconds kHealthPeriod(2);

// (system_clock: the wait is pthread_cond_timedwait, which every
// ThreadSanitizer runtime intercepts; a clock step only moves one wake-up)
std::chrono::system_clock::time_point nextHealthCheck() {
  return std::chrono::system_clock::now() + kHealthPeriod;
}

}  // namespace

Stager::Stager(StagerConfig cfg) : cfg_(std::move(cfg)) {
  if (cfg_.numWorkers <= 0 || cfg_.batchSize <= 0 || cfg_.numBatches <= 0 ||
      cfg_.numSlots < 2 || cfg_.doneSems == nullptr || !cfg_.prepare || !cfg_.failure) {
    throw std::invalid_argument("stager: bad configuration");
  }
  batches_.resize(cfg_.numBatches);
  for (Batch& b : batches_) b.slots.assign(cfg_.numSlots, SlotState::Free);
  stagedSlot_.reset(new std::atomic<int>[cfg_.numBatches]);
  for (int b = 0; b < cfg_.numBatches; ++b) stagedSlot_[b].store(-1);
  thread_ = std::thread([this] { run(); });
}

Stager::~Stager() {
  {
    std::lock_guard<std::mutex> lk(mu_);
    stop_ = true;
  }
  stopFlag_.store(true, std::memory_order_release);
  cv_.notify_all();
  if (thread_.joinable()) thread_.join();
}

std::string Stager::submit(int b) {
  if (b < 0 || b >= cfg_.numBatches) return "stager: bad batch index";
  {
    std::lock_guard<std::mutex> lk(mu_);
    Batch& B = batches_[b];
    if (B.queued > 0 || stagedSlot_[b].load(std::memory_order_relaxed) >= 0) {
      return "envpool: batch " + std::to_string(b) +
             " stepped again before its staged result was consumed";
    }
    ++B.queued;
    queue_.push_back(b);
  }
  cv_.notify_all();
  return "";
}

bool Stager::ready(int b) const {
  if (b < 0 || b >= cfg_.numBatches) return false;
  return stagedSlot_[b].load(std::memory_order_acquire) >= 0 ||
         failed_.load(std::memory_order_acquire);
}

int Stager::wait(int b, std::string* error) {
  if (b < 0 || b >= cfg_.numBatches) {
    *error = "stager: bad batch index";
    return -1;
  }
  std::unique_lock<std::mutex> lk(mu_);
  Batch& B = batches_[b];
  while (true) {
    if (!error_.empty()) {
      *error = error_;
      return -1;
    }
    int s = stagedSlot_[b].load(std::memory_order_relaxed);
    if (s >= 0) {
      B.slots[s] = SlotState::Held;
      stagedSlot_[b].store(-1, std::memory_order_release);
      return s;
    }
    if (stop_) {
      *error = "envpool: staging stopped";
      return -1;
    }
    if (B.queued == 0) {
      *error = "envpool: result of batch " + std::to_string(b) + " requested before its step";
      return -1;
    }
    // the stager thread does the health checks and notifies on failure
    cv_.wait_until(lk, nextHealthCheck());
  }
}

std::string Stager::release(int b, int slot) {
  if (b < 0 || b >= cfg_.numBatches || slot < 0 || slot >= cfg_.numSlots) {
    return "stager: bad batch or slot index";
  }
  {
    std::lock_guard<std::mutex> lk(mu_);
    SlotState& st = batches_[b].slots[slot];
    if (st != SlotState::Held) {
      return "envpool: release of slot " + std::to_string(slot) + " of batch " +
             std::to_string(b) + ", which no result() handed out";
    }
    st = SlotState::Free;
  }
  cv_.notify_all();
  return "";
}

void Stager::fail(const std::string& msg) {
  {
    std::lock_guard<std::mutex> lk(mu_);
    if (error_.empty()) error_ = msg;
  }
  failed_.store(true, std::memory_order_release);
  cv_.notify_all();
}

void Stager::run() {
  while (true) {
    int b;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [this] { return stop_ || !queue_.empty(); });
      if (stop_) return;
      b = queue_.front();
      queue_.pop_front();
    }
    // after a failure nothing more is staged: every later wait() reports it
    if (!failed_.load(std::memory_order_relaxed)) stageOne(b);
  }
}

void Stager::stageOne(int b) {
  // 1. the slot: blocks on the consumer's release(), and on nothing else
  int slot;
  {
    std::unique_lock<std::mutex> lk(mu_);
    Batch& B = batches_[b];
    slot = B.nextSlot;
    while (!stop_ && B.slots[slot] != SlotState::Free) {
      if (cv_.wait_until(lk, nextHealthCheck()) == std::cv_status::timeout) {
        lk.unlock();
        std::string msg = cfg_.failure();
        if (!msg.empty()) {
          fail(msg);
          return;
        }
        lk.lock();
      }
    }
    if (stop_) return;
    B.slots[slot] = SlotState::Filling;
    B.nextSlot = (slot + 1) % cfg_.numSlots;
  }

  // 2. the workers: copy each one's rows as soon as it has posted
  const int W = cfg_.numWorkers;
  std::vector<char> copied(W, 0);
  int remaining = W;
  auto take = [&](int w) -> bool {
    if (!planned_) {
      std::string msg = cfg_.prepare(plan_);
      if (msg.empty() && plan_.size() != static_cast<size_t>(cfg_.numBatches)) {
        msg = "stager: plan does not cover every batch";
      }
      for (size_t i = 0; msg.empty() && i < plan_.size(); ++i) {
        if (plan_[i].size() != static_cast<size_t>(cfg_.numSlots)) {
          msg = "stager: plan does not cover every slot";
        }
      }
      if (!msg.empty()) {
        fail(msg);
        return false;
      }
      planned_ = true;
    }
    copyWorkerRows(b, slot, w);
    copied[w] = 1;
    --remaining;
    return true;
  };
  while (remaining > 0) {
    bool progressed = false;
    int firstPending = -1;
    for (int w = 0; w < W; ++w) {
      if (copied[w]) continue;
      if (sem_trywait(&cfg_.doneSems[b * W + w]) == 0) {
        if (!take(w)) return;
        progressed = true;
      } else if (firstPending < 0) {
        firstPending = w;
      }
    }
    if (progressed || firstPending < 0) continue;
    if (!waitWorker(b, firstPending)) return;
    if (!take(firstPending)) return;
  }

  // 3. publish
  {
    std::lock_guard<std::mutex> lk(mu_);
    Batch& B = batches_[b];
    B.slots[slot] = SlotState::Staged;
    --B.queued;
    stagedSlot_[b].store(slot, std::memory_order_release);
  }
  cv_.notify_all();
}

bool Stager::waitWorker(int b, int w) {
  sem_t* sem = &cfg_.doneSems[b * cfg_.numWorkers + w];
  for (int slice = 1;; ++slice) {
    timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    ts.tv_nsec += kSliceMs * 1000 * 1000;
    if (ts.tv_nsec >= 1000000000) {
      ts.tv_sec += 1;
      ts.tv_nsec -= 1000000000;
    }
    if (sem_timedwait(sem, &ts) == 0) return true;
    if (stopFlag_.load(std::memory_order_acquire)) return false;
    if (errno == EINTR) continue;
    if (slice % kHealthEvery == 0) {
      std::string msg = cfg_.failure();
      if (!msg.empty()) {
        fail(msg);
        return false;
      }
    }
  }
}

void Stager::copyWorkerRows(int b, int slot, int w) {
  // worker w owns envs w, w + numWorkers, ... (EnvPool::workerMain)
  for (const StagerCopy& c : plan_[b][slot]) {
    for (int e = w; e < cfg_.batchSize; e += cfg_.numWorkers) {
      size_t off = static_cast<size_t>(e) * c.bytesPerEnv;
      std::memcpy(c.dst + off, c.src + off, c.bytesPerEnv);
    }
  }
}

}  // namespace mrl
