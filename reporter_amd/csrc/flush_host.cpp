// flush_host.cpp -- the datastore flush body written on the host.
//
// reporter_amd/datastore.py's serialize(flush_records(...)) in C: the
// statement of the format that needs no GPU, the answer for a slice the device
// writer (flush.hip) declines, and the path of a host that reduced its
// histograms on the CPU.  No HIP call and no engine in here: the file links
// with json.cpp alone (tests/native/flush_host_main.c).
#define OTM_FLUSH_HOST_ONLY
#include "flush.h"

#include <charconv>
#include <cstdlib>
#include <cstring>
#include <new>

#include "json.h"
#include "otmatch.h"

// abi.cpp's thread error (otm_last_error); absent where this file links alone
extern "C" __attribute__((weak, visibility("hidden"))) void otm_set_last_error(const char* msg);

namespace otm {

static void put_u64(uint64_t v, std::string* o) {
  char buf[24];
  auto r = std::to_chars(buf, buf + sizeof buf, v);
  o->append(buf, r.ptr);
}

std::string flush_head(float bin_kph, int rank, int world) {
  std::string o = "{\"mode\":\"auto\",\"bin_kph\":";
  json::put_float((double)bin_kph, &o);
  o += ",\"rank\":";
  json::put_int(rank, &o);
  o += ",\"world\":";
  json::put_int(world, &o);
  o += ",\"segments\":[";
  return o;
}

int flush_body_host(const uint32_t* counts, const uint64_t* speed_sum, const uint64_t* segment_ids,
                    int64_t n_segments, int64_t rows, int nbins, float bin_kph, int rank, int world, char** body,
                    size_t* body_len, int64_t* n_records, std::string* err) {
  if (!body || !body_len) {
    *err = "body and body_len must not be NULL";
    return OTM_EINVAL;
  }
  *body = nullptr;
  *body_len = 0;
  if (n_records) *n_records = 0;
  if (rows < 0 || n_segments < 0 || (rows > 0 && (!counts || !speed_sum)) || (n_segments > 0 && !segment_ids)) {
    *err = "counts, speed_sum and segment_ids must not be NULL";
    return OTM_EINVAL;
  }
  if (nbins < 1 || !(bin_kph > 0.0f)) {
    *err = "nbins >= 1 and bin_kph > 0";
    return OTM_EINVAL;
  }
  if (world < 1 || rank < 0 || rank >= world) {
    *err = "world >= 1 and 0 <= rank < world";
    return OTM_EINVAL;
  }
  try {
    std::string o = flush_head(bin_kph, rank, world);
    int64_t n = 0;
    const int64_t row0 = (int64_t)rank * rows;
    for (int64_t k = 0; k < rows && row0 + k < n_segments; ++k) {  // (padding rows carry no id)
      const uint32_t* c = counts + k * (int64_t)nbins;
      uint64_t tot = 0;
      for (int b = 0; b < nbins; ++b) tot += c[b];
      if (!tot) continue;
      o += n ? ",{\"id\":" : "{\"id\":";
      put_u64(segment_ids[row0 + k], &o);
      o += ",\"count\":";
      put_u64(tot, &o);
      o += ",\"speed_sum_kph\":";
      // Python's int / float: the integer rounded to a double, one IEEE division
      json::put_float((double)speed_sum[k] / 1000.0, &o);
      o += ",\"bins\":[";
      for (int b = 0; b < nbins; ++b) {
        if (b) o += ',';
        put_u64(c[b], &o);
      }
      o += "]}";
      ++n;
    }
    o += "]}";
    char* p = (char*)std::malloc(o.size() + 1);
    if (!p) throw std::bad_alloc();
    std::memcpy(p, o.data(), o.size());
    p[o.size()] = '\0';
    *body = p;
    *body_len = o.size();
    if (n_records) *n_records = n;
    return OTM_OK;
  } catch (const std::bad_alloc&) {
    *err = "out of host memory";
    return OTM_ENOMEM;
  }
}

}  // namespace otm

extern "C" int otm_flush_body_host(const uint32_t* counts, const uint64_t* speed_sum, const uint64_t* segment_ids,
                                   int64_t n_segments, int64_t rows, int nbins, float bin_kph, int rank, int world,
                                   char** body, size_t* body_len, int64_t* n_records) {
  std::string err;
  const int rc = otm::flush_body_host(counts, speed_sum, segment_ids, n_segments, rows, nbins, bin_kph, rank, world,
                                      body, body_len, n_records, &err);
  if (rc && otm_set_last_error) otm_set_last_error(err.c_str());
  return rc;
}
