// Stand-alone race check for csrc/stager.{h,cc}: no Python, no torch, no GPU.
//
// Threads stand in for the EnvPool's worker processes. They fill their rows
// of a batch in an anonymous shared mapping and post process-shared POSIX
// semaphores that live in the same mapping, exactly as the pool's workers do.
// The main thread is the consumer (submit / wait / verify), and a third kind
// of thread hands slots back after random delays, so release() races with
// the stager's slot wait and with the consumer's wait().
//
// Build and run under the sanitizers (from the repository root):
//   g++ -std=c++17 -O1 -g -fsanitize=thread -Icsrc tools/stager_race.cc \
//       csrc/stager.cc -o /tmp/stager_race_tsan -pthread && /tmp/stager_race_tsan
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc tools/stager_race.cc \
//       csrc/stager.cc -o /tmp/stager_race_asan -pthread && /tmp/stager_race_asan
// Optional argument: steps per configuration (default 2000).
// Exit status 0 and "stager_race: ok" mean every staged byte was right, the
// slots alternated, and held slots were never written.
#include <semaphore.h>
#include <sys/mman.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "stager.h"

namespace {

constexpr int kSlots = 2;
constexpr size_t kObsBytes = 37;  // odd on purpose
constexpr size_t kFieldBytes[3] = {kObsBytes, sizeof(float), 1};

unsigned char obsByte(int env, int step, size_t j) {
  return static_cast<unsigned char>(env * 131 + step * 7 + static_cast<int>(j));
}
float rewardOf(int env, int step) { return static_cast<float>(env + 1000 * step); }
unsigned char doneOf(int env, int step) { return (env + step) % 3 == 0 ? 1 : 0; }

struct WorkQueue {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<int> items;  // batch index, -1 = exit
  void push(int b) {
    {
      std::lock_guard<std::mutex> lk(mu);
      items.push_back(b);
    }
    cv.notify_one();
  }
  int pop() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this] { return !items.empty(); });
    int b = items.front();
    items.pop_front();
    return b;
  }
};

struct Release {
  int b, slot, delayUs;
};

std::atomic<int> fails{0};
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fprintf(stderr, "\n");       \
      ++fails;                          \
    }                                   \
  } while (0)

bool runConfig(int batchSize, int W, int numBatches, int steps, unsigned seed) {
  size_t bytesPerBatch = 0;
  size_t fieldOff[3];
  for (int f = 0; f < 3; ++f) {
    fieldOff[f] = bytesPerBatch;
    bytesPerBatch += ((kFieldBytes[f] * batchSize + 63) / 64) * 64;
  }
  size_t semBytes = ((sizeof(sem_t) * numBatches * W + 63) / 64) * 64;
  size_t total = semBytes + bytesPerBatch * numBatches;
  char* base = static_cast<char*>(
      mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0));
  if (base == MAP_FAILED) {
    std::perror("mmap");
    return false;
  }
  sem_t* sems = reinterpret_cast<sem_t*>(base);
  for (int i = 0; i < numBatches * W; ++i) sem_init(&sems[i], 1, 0);
  auto src = [&](int b, int f) { return base + semBytes + bytesPerBatch * b + fieldOff[f]; };

  // staging slots: ordinary heap memory, one buffer per (batch, slot, field)
  std::vector<std::vector<std::vector<std::vector<char>>>> slots(numBatches);
  for (int b = 0; b < numBatches; ++b) {
    slots[b].resize(kSlots);
    for (int s = 0; s < kSlots; ++s) {
      for (int f = 0; f < 3; ++f) slots[b][s].emplace_back(kFieldBytes[f] * batchSize, '\xee');
    }
  }

  std::atomic<bool> failNow{false};
  mrl::StagerConfig cfg;
  cfg.numWorkers = W;
  cfg.batchSize = batchSize;
  cfg.numBatches = numBatches;
  cfg.numSlots = kSlots;
  cfg.doneSems = sems;
  cfg.prepare = [&](mrl::StagerPlan& plan) -> std::string {
    plan.assign(numBatches, {});
    for (int b = 0; b < numBatches; ++b) {
      for (int s = 0; s < kSlots; ++s) {
        std::vector<mrl::StagerCopy> copies;
        for (int f = 0; f < 3; ++f) {
          mrl::StagerCopy c;
          c.src = src(b, f);
          c.dst = slots[b][s][f].data();
          c.bytesPerEnv = kFieldBytes[f];
          copies.push_back(c);
        }
        plan[b].push_back(std::move(copies));
      }
    }
    return "";
  };
  cfg.failure = [&]() -> std::string { return failNow.load() ? "worker 0 died" : ""; };

  // workers
  std::vector<WorkQueue> queues(W);
  std::vector<std::thread> workers;
  for (int w = 0; w < W; ++w) {
    workers.emplace_back([&, w] {
      std::mt19937 rng(seed * 977 + w);
      std::vector<int> step(numBatches, 0);
      while (true) {
        int b = queues[w].pop();
        if (b < 0) return;
        if (rng() % 4 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 150));
        for (int e = w; e < batchSize; e += W) {
          char* o = src(b, 0) + kObsBytes * e;
          for (size_t j = 0; j < kObsBytes; ++j) o[j] = static_cast<char>(obsByte(e, step[b], j));
          float r = rewardOf(e, step[b]);
          std::memcpy(src(b, 1) + sizeof(float) * e, &r, sizeof(float));
          src(b, 2)[e] = static_cast<char>(doneOf(e, step[b]));
        }
        ++step[b];
        sem_post(&sems[b * W + w]);
      }
    });
  }

  bool ok = true;
  {
    mrl::Stager stager(cfg);

    // releaser thread
    std::mutex rmu;
    std::condition_variable rcv;
    std::deque<Release> rq;
    bool rstop = false;
    std::thread releaser([&] {
      while (true) {
        Release r;
        {
          std::unique_lock<std::mutex> lk(rmu);
          rcv.wait(lk, [&] { return rstop || !rq.empty(); });
          if (rq.empty()) return;
          r = rq.front();
          rq.pop_front();
        }
        if (r.delayUs) std::this_thread::sleep_for(std::chrono::microseconds(r.delayUs));
        std::string err = stager.release(r.b, r.slot);
        CHECK(err.empty(), "release failed: %s", err.c_str());
      }
    });

    auto verify = [&](int b, int slot, int step, const char* when) {
      for (int e = 0; e < batchSize; ++e) {
        const char* o = slots[b][slot][0].data() + kObsBytes * e;
        for (size_t j = 0; j < kObsBytes; ++j) {
          if (static_cast<unsigned char>(o[j]) != obsByte(e, step, j)) {
            CHECK(false, "%s: obs mismatch batch %d slot %d env %d step %d byte %zu", when, b,
                  slot, e, step, j);
            return;
          }
        }
        float r;
        std::memcpy(&r, slots[b][slot][1].data() + sizeof(float) * e, sizeof(float));
        CHECK(r == rewardOf(e, step), "%s: reward mismatch batch %d env %d step %d", when, b, e,
              step);
        CHECK(static_cast<unsigned char>(slots[b][slot][2][e]) == doneOf(e, step),
              "%s: done mismatch batch %d env %d step %d", when, b, e, step);
      }
    };

    auto post = [&](int b) {
      std::string err = stager.submit(b);
      CHECK(err.empty(), "submit failed: %s", err.c_str());
      for (int w = 0; w < W; ++w) queues[w].push(b);
    };

    std::mt19937 rng(seed);
    std::vector<int> step(numBatches, 0), held(numBatches, -1), heldStep(numBatches, -1);
    for (int b = 0; b < numBatches; ++b) post(b);
    for (int i = 0; i < steps && fails == 0; ++i) {
      int b = i % numBatches;
      if (rng() % 8 == 0) {  // poll like the training loop does
        while (!stager.ready(b)) std::this_thread::yield();
      }
      std::string err;
      int slot = stager.wait(b, &err);
      CHECK(slot >= 0, "wait failed: %s", err.c_str());
      if (slot < 0) break;
      CHECK(slot == step[b] % kSlots, "slot %d at step %d of batch %d: not ping-pong", slot,
            step[b], b);
      verify(b, slot, step[b], "fresh");
      // the previous slot of this batch stayed ours while this one was filled
      if (held[b] >= 0) {
        verify(b, held[b], heldStep[b], "held");
        std::lock_guard<std::mutex> lk(rmu);
        rq.push_back({b, held[b], (rng() % 3 == 0) ? static_cast<int>(rng() % 300) : 0});
      }
      rcv.notify_one();
      held[b] = slot;
      heldStep[b] = step[b];
      ++step[b];
      if (rng() % 5 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 100));
      post(b);
    }
    // drain: one result per batch is still in flight
    for (int b = 0; b < numBatches && fails == 0; ++b) {
      if (held[b] >= 0) {
        std::lock_guard<std::mutex> lk(rmu);
        rq.push_back({b, held[b], 0});
      }
      rcv.notify_one();
      std::string err;
      int slot = stager.wait(b, &err);
      CHECK(slot >= 0, "drain wait failed: %s", err.c_str());
      if (slot >= 0) {
        verify(b, slot, step[b], "drain");
        std::lock_guard<std::mutex> lk(rmu);
        rq.push_back({b, slot, 0});
      }
      rcv.notify_one();
    }
    {
      std::lock_guard<std::mutex> lk(rmu);
      rstop = true;
    }
    rcv.notify_all();
    releaser.join();

    // failure path: work that no worker ever finishes, then an unhealthy pool
    if (fails == 0) {
      std::string err = stager.submit(0);
      CHECK(err.empty(), "submit failed: %s", err.c_str());
      failNow.store(true);
      auto t0 = std::chrono::steady_clock::now();
      int slot = stager.wait(0, &err);
      double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      CHECK(slot < 0 && err == "worker 0 died", "failure not reported (slot %d, '%s')", slot,
            err.c_str());
      CHECK(dt < 5.0, "failure took %.1f s to surface", dt);
      CHECK(stager.ready(0), "ready() false after a failure");
    }
    ok = fails == 0;
    // ~Stager joins the thread while it may be blocked: must not hang
  }
  for (int w = 0; w < W; ++w) queues[w].push(-1);
  for (std::thread& t : workers) t.join();
  for (int i = 0; i < numBatches * W; ++i) sem_destroy(&sems[i]);
  munmap(base, total);
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  int steps = argc > 1 ? std::atoi(argv[1]) : 2000;
  const int configs[][3] = {{5, 2, 2}, {1, 1, 1}, {7, 3, 2}, {8, 8, 1}, {128, 10, 2}};
  unsigned seed = 1;
  for (const auto& c : configs) {
    bool ok = runConfig(c[0], c[1], c[2], steps, seed++);
    std::printf("stager_race: batch %d workers %d batches %d steps %d: %s\n", c[0], c[1], c[2],
                steps, ok ? "ok" : "FAILED");
    if (!ok) return 1;
  }
  std::printf("stager_race: ok\n");
  return 0;
}
