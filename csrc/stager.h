// Stager: one native thread per EnvPool that copies finished env results out
// of the shared-memory segment into caller-supplied staging slots.
//
// The consumer (the Python thread that drives training) would otherwise copy
// every result itself: a host-to-device copy from the pageable segment runs
// on the calling thread. The stager does that copy on a thread that never
// takes the GIL, into slots the caller allocated (pinned on a GPU machine),
// so the consumer's later copy to the device is a truly asynchronous DMA.
//
// Per submitted batch the thread
//   1. blocks until the batch's next slot (ping-pong order) has been released,
//   2. waits on the per-(batch, worker) completion semaphores itself and, as
//      each worker posts, copies that worker's rows of every field,
//   3. publishes "batch b staged in slot s" (atomic + condition variable).
// Every wait wakes after 2 s to ask the owner whether a worker failed or
// died; a failure is stored and handed to the consumer by wait().
//
// This file has no Python, torch or HIP dependency: the pool supplies plain
// pointers, and tools/stager_race.cc drives it stand-alone under sanitizers.
#pragma once

#include <semaphore.h>

#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace mrl {

// One field of one (batch, slot): rows of bytesPerEnv bytes, row e at e * bytesPerEnv.
struct StagerCopy {
  const char* src = nullptr;
  char* dst = nullptr;
  size_t bytesPerEnv = 0;
};

// copies[batch][slot] = one StagerCopy per field.
using StagerPlan = std::vector<std::vector<std::vector<StagerCopy>>>;

struct StagerConfig {
  int numWorkers = 0;
  int batchSize = 0;
  int numBatches = 0;
  int numSlots = 0;            // per batch, >= 2
  sem_t* doneSems = nullptr;   // [numBatches * numWorkers], posted by the workers
  // Called once on the stager thread, after the first worker has posted (the
  // field layout is published by then). Fills the plan; returns "" or an error.
  std::function<std::string(StagerPlan&)> prepare;
  // Health check run at every 2 s wake-up: "" or the failure to report.
  std::function<std::string()> failure;
};

class Stager {
 public:
  explicit Stager(StagerConfig cfg);  // starts the thread
  ~Stager();                          // stops and joins it
  Stager(const Stager&) = delete;
  Stager& operator=(const Stager&) = delete;

  // The workers are being handed batch b: stage it when they finish. Returns
  // "" or why the call is invalid (b's previous result is still unconsumed).
  std::string submit(int b);
  // True iff batch b is staged and not yet consumed, or staging has failed.
  bool ready(int b) const;
  // Blocks until ready(b). Returns the slot and consumes the result, or
  // returns -1 with *error set. The slot stays the consumer's until release().
  int wait(int b, std::string* error);
  // Hands a consumed slot back. Returns "" or why the call is invalid.
  std::string release(int b, int slot);

 private:
  enum class SlotState : uint8_t { Free, Filling, Staged, Held };
  struct Batch {
    std::vector<SlotState> slots;
    int nextSlot = 0;
    int queued = 0;  // submitted, not yet staged
  };

  void run();
  void stageOne(int b);
  bool waitWorker(int b, int w);  // false: stopped or failed
  void copyWorkerRows(int b, int slot, int w);
  void fail(const std::string& msg);

  StagerConfig cfg_;
  StagerPlan plan_;
  bool planned_ = false;  // stager thread only

  mutable std::mutex mu_;
  std::condition_variable cv_;
  std::deque<int> queue_;
  std::vector<Batch> batches_;
  std::string error_;
  bool stop_ = false;
  // lock-free mirrors for ready(): staged slot per batch (-1 none), failure flag
  std::unique_ptr<std::atomic<int>[]> stagedSlot_;
  std::atomic<bool> failed_{false};
  std::atomic<bool> stopFlag_{false};

  std::thread thread_;
};

}  // namespace mrl
