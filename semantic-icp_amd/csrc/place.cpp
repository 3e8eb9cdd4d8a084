// place.cpp -- sicp_place_* (include/sicp.h): a database of scan descriptors that lives on the device between calls.  The
// entries lie one after another in one of two arena buffers; growth doubles into the spare buffer and swaps last, so a refused
// call leaves the entries as they were by construction.  The kernels: place_kernels.hip and the radix sort of prim_kernels.hip.
#include "engine.hpp"

namespace sicp {
namespace host {
namespace {

#define PLACECHECK(expr)                                                                       \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      db->last_error = std::string(db->call) + ": " #expr ": " + hipGetErrorString(_e) +       \
                       "; the database is unchanged";                                          \
      return _e == hipErrorOutOfMemory ? SICP_ERR_OUT_OF_MEMORY : SICP_ERR_HIP;                \
    }                                                                                          \
  } while (0)

constexpr double kTwoPi = 6.283185307179586;

// A call's device scratch: taken from the arena, given back at the end (`idle`: the stream has been synchronised behind the
// call's launches).
struct PlaceScratch {
  DevBuf<unsigned char> temp;
  DevBuf<uint32_t> table;
  DevBuf<unsigned long long> res, key, key2, hit;
  DevBuf<int4> rows;
  int device = -1;
  bool idle = true;
  ~PlaceScratch() { DevArena::release_scratch(device, idle, temp, table, res, key, key2, hit, rows); }
};

bool slot_ok(int which) { return which == SICP_SOURCE || which == SICP_TARGET; }
bool is_label(const sicp_place_ctx* db) { return db->params.channel == SICP_PLACE_LABEL; }

bool params_ok(const sicp_place_params& p) {
  if (p.n_rings < 1 || p.n_rings > sicp::kPlaceMaxRings) return false;
  if (p.n_sectors < 4 || p.n_sectors > sicp::kPlaceMaxSectors || p.n_sectors % 4 != 0) return false;
  if (!std::isfinite(p.max_range) || !(p.max_range > 0.0)) return false;
  if (!(p.min_range >= 0.0) || !(p.min_range < p.max_range)) return false;
  if (p.min_cell_points < 1) return false;
  if (p.channel == SICP_PLACE_LABEL) {
    if (p.num_classes < 1 || p.num_classes > 255) return false;
    if (p.n_ignore < 0 || p.n_ignore > SICP_PLACE_MAX_IGNORE) return false;
    for (int j = 0; j < p.n_ignore; ++j)
      if (p.ignore[j] < 1 || p.ignore[j] > (uint32_t)p.num_classes) return false;
    return true;
  }
  // (a z_step so small that its reciprocal overflows would turn dz == z_min into 0 * inf)
  if (p.channel == SICP_PLACE_HEIGHT) return std::isfinite(p.z_min) && std::isfinite(p.z_step) && p.z_step > 0.0 && std::isfinite(1.0 / p.z_step);
  return false;
}

// the first byte of desc[0 .. bytes) above the class count of a LABEL database, or -1
long long first_bad_byte(const sicp_place_ctx* db, const uint8_t* desc, size_t bytes) {
  if (!is_label(db) || db->params.num_classes >= 255) return -1;
  const uint8_t C = (uint8_t)db->params.num_classes;
  for (size_t i = 0; i < bytes; ++i)
    if (desc[i] > C) return (long long)i;
  return -1;
}

std::string bad_byte_text(const sicp_place_ctx* db, const uint8_t* desc, long long at) {
  const long long rs = db->rs, S = db->params.n_sectors;
  return "descriptor " + std::to_string(at / rs) + ", ring " + std::to_string(at % rs / S) + ", sector " + std::to_string(at % S) + " (byte " +
         std::to_string(at) + ") is " + std::to_string((int)desc[at]) + ", above num_classes = " + std::to_string(db->params.num_classes);
}

// the checks of a call that reads a slot, before any device work; `why` gets the refusal
int check_slot(const sicp_place_ctx* db, const sicp_context* h, int which, const double* sensor_origin, std::string& why) {
  if (!h) { why = "the handle is NULL"; return SICP_ERR_INVALID_ARGUMENT; }
  if (!slot_ok(which)) { why = "`which` is neither SICP_SOURCE nor SICP_TARGET"; return SICP_ERR_INVALID_ARGUMENT; }
  if (h->device != db->device) {
    why = "the handle is on device " + std::to_string(h->device) + ", the database on " + std::to_string(db->device);
    return SICP_ERR_INVALID_ARGUMENT;
  }
  if (sensor_origin)
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(sensor_origin[d])) { why = "sensor_origin must be finite"; return SICP_ERR_INVALID_ARGUMENT; }
  return SICP_OK;
}

// first / count of a query or a get against the size: count = -1 becomes "to the end"
int resolve_range(const sicp_place_ctx* db, int32_t first, int32_t& count, std::string& why) {
  const long long size = db->n_entries;
  if (first < 0) { why = "first = " + std::to_string(first) + " is negative"; return SICP_ERR_INVALID_ARGUMENT; }
  if (count < -1) { why = "count = " + std::to_string(count) + " is neither -1 nor a number of entries"; return SICP_ERR_INVALID_ARGUMENT; }
  if ((long long)first > size || (count >= 0 && (long long)first + count > size)) {
    why = "the range " + std::to_string(first) + " + " + std::to_string(count) + " reaches beyond the " + std::to_string(size) + " entries";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  if (count < 0) count = (int32_t)(size - first);
  return SICP_OK;
}

// The descriptor of the slot into db->qdesc (device) and db->stage (pinned: the result words, then the R*S bytes).  Every check
// has been made but the cloud's; leaves the stream idle.  `call` names the entry point in the error text.
int describe_device(sicp_place_ctx* db, const char* call, sicp_context* h, int which, const double* sensor_origin,
                    sicp_place_describe_info& I) {
  const std::string name = call;
  Cloud& c = h->cloud(which);
  if (!c.is_set) {
    db->last_error = name + ": the slot has no cloud";
    return SICP_ERR_NOT_READY;
  }
  const bool lab = is_label(db);
  if (lab && !c.has_label) {
    db->last_error = name + ": the cloud has no labels and the database describes scans by label; nothing was done";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  PLACECHECK(hipSetDevice(db->device));
  if (c.layout < 0) {  // (prepared as a merge part is: sicp_map_integrate's rule)
    const int rc = prepare_cloud(h, c);
    if (rc != SICP_OK) {
      db->last_error = name + ": the cloud: " + (h->last_error.empty() ? std::string("not ready") : h->last_error);
      return rc;
    }
  }
  if (c.pending && c.ready_ev) {  // (the upload runs on the handle's stream, the kernels below on the database's)
    PLACECHECK(hipEventSynchronize(c.ready_ev));
    c.pending = false;
  }
  const sicp_place_params& P = db->params;
  const size_t rs = (size_t)db->rs;
  const size_t table_words = rs * (size_t)(lab ? P.num_classes : 2);
  hipStream_t st = db->stream;
  PlaceScratch X;
  X.device = db->device;
  X.idle = false;
  const size_t head = sizeof(unsigned long long) * sicp::kPlaceRes;
  PLACECHECK(db->stage.resize(head + rs));
  PLACECHECK(db->qdesc.reserve(rs));
  PLACECHECK(X.table.reserve(table_words));
  PLACECHECK(X.res.reserve(sicp::kPlaceRes));
  sicp::PlaceDescribeArgs A;
  std::memset(&A, 0, sizeof A);
  A.x = c.rx.p; A.y = c.ry.p; A.z = c.rz.p;
  A.label = lab ? c.rl.p : nullptr;
  A.n = c.n; A.R = P.n_rings; A.S = P.n_sectors; A.C = lab ? P.num_classes : 0;
  A.ox = sensor_origin ? (float)sensor_origin[0] : 0.f;
  A.oy = sensor_origin ? (float)sensor_origin[1] : 0.f;
  A.oz = sensor_origin ? (float)sensor_origin[2] : 0.f;
  A.min_range_sq = P.min_range * P.min_range;
  A.z_min = P.z_min;
  A.inv_z_step = lab ? 0.0 : 1.0 / P.z_step;
  A.tables = db->d_tables.p;
  if (lab)
    for (int j = 0; j < P.n_ignore; ++j) A.ignore[P.ignore[j] >> 5] |= 1u << (P.ignore[j] & 31);
  A.min_cell_points = P.min_cell_points;
  A.table = X.table.p; A.desc = db->qdesc.p; A.res = X.res.p;
  PLACECHECK(hipMemsetAsync(X.table.p, 0, sizeof(uint32_t) * table_words, st));
  PLACECHECK(hipMemsetAsync(X.res.p, 0, head, st));
  PLACECHECK(sicp::launch_place_cells(A, st));
  PLACECHECK(sicp::launch_place_finalise(A, st));
  PLACECHECK(hipMemcpyAsync(db->stage.data(), X.res.p, head, hipMemcpyDeviceToHost, st));
  PLACECHECK(hipMemcpyAsync(db->stage.data() + head, db->qdesc.p, rs, hipMemcpyDeviceToHost, st));
  PLACECHECK(hipStreamSynchronize(st));
  X.idle = true;
  unsigned long long res[sicp::kPlaceRes];
  std::memcpy(res, db->stage.data(), head);
  if (res[sicp::kPlaceBadLabel]) {
    db->last_error = name + ": a kept point's label is above num_classes = " + std::to_string(P.num_classes) + "; nothing was done";
    return SICP_ERR_BAD_LABEL;
  }
  std::memset(&I, 0, sizeof I);
  I.n_in = c.n;
  I.n_kept = (int64_t)res[sicp::kPlaceKept];
  I.n_cells = (int32_t)res[sicp::kPlaceCells];
  return SICP_OK;
}
const uint8_t* staged_desc(const sicp_place_ctx* db) { return db->stage.data() + sizeof(unsigned long long) * sicp::kPlaceRes; }

// Room for n more entries: the spare buffer at twice the capacity, the entries copied over, the swap last.  Leaves the stream
// idle.
int grow_for(sicp_place_ctx* db, long long n) {
  const long long need = db->n_entries + n;
  if (need <= db->cap_entries) return SICP_OK;
  const size_t rs = (size_t)db->rs;
  const long long want = std::max<long long>(std::max<long long>(need, 2 * db->cap_entries), 64);
  DevBuf<uint8_t>& cur = db->store[db->cur];
  DevBuf<uint8_t>& spare = db->store[db->cur ^ 1];
  PLACECHECK(spare.reserve((size_t)want * rs));
  if (db->n_entries > 0) {
    PLACECHECK(hipMemcpyAsync(spare.p, cur.p, (size_t)db->n_entries * rs, hipMemcpyDeviceToDevice, db->stream));
    PLACECHECK(hipStreamSynchronize(db->stream));
  }
  db->cur ^= 1;
  db->cap_entries = want;
  {
    DevArena::FreeScope idle(db->device);  // (nothing reads the old buffer any more)
    cur.release();
  }
  return SICP_OK;
}

// The search of queries db->qdesc[0 .. n_q) against entries first .. first+count-1 (count resolved, every argument checked).
int search_device(sicp_place_ctx* db, int32_t n_q, int32_t first, int32_t count, int32_t top_k, double min_score, sicp_place_candidate* out,
                  int32_t* n_found) {
  if (count == 0) {  // (an empty range or database)
    for (int q = 0; q < n_q; ++q) n_found[q] = 0;
    return SICP_OK;
  }
  const int S = db->params.n_sectors;
  const size_t rs = (size_t)db->rs;
  const int top = std::min(top_k, count);
  const size_t pairs = (size_t)n_q * (size_t)count, n_rows = (size_t)n_q * (size_t)top;
  PLACECHECK(hipSetDevice(db->device));
  hipStream_t st = db->stream;
  PlaceScratch X;
  X.device = db->device;
  X.idle = false;
  PLACECHECK(db->stage.resize(sizeof(int4) * n_rows));
  PLACECHECK(X.key.reserve(pairs)); PLACECHECK(X.key2.reserve(pairs)); PLACECHECK(X.hit.reserve(pairs));
  PLACECHECK(X.rows.reserve(n_rows));
  size_t sort_bytes = 0;
  PLACECHECK(sicp::prim_sort_keys(nullptr, sort_bytes, X.key.p, X.key2.p, count, 0, 62, st));
  PLACECHECK(X.temp.reserve(sort_bytes + 256));
  sicp::PlaceSearchArgs A;
  std::memset(&A, 0, sizeof A);
  A.query = db->qdesc.p;
  A.entries = db->store[db->cur].p + (size_t)first * rs;
  A.n_q = n_q; A.count = count; A.R = db->params.n_rings; A.S = S;
  A.key = X.key.p; A.hit = X.hit.p;
  PLACECHECK(sicp::launch_place_search(A, st));
  // ascending keys: the best score first, the smallest id first among equals.  One sort launch per query: rocPRIM's segmented
  // sort gives a segment to one workgroup (4 ms for 100 000 keys), which is no use for a query's keys
  for (int q = 0; q < n_q; ++q)
    PLACECHECK(sicp::prim_sort_keys(X.temp.p, sort_bytes, X.key.p + (size_t)q * count, X.key2.p + (size_t)q * count, count, 0, 62, st));
  PLACECHECK(sicp::launch_place_gather(X.key2.p, X.hit.p, n_q, count, top, X.rows.p, st));
  PLACECHECK(hipMemcpyAsync(db->stage.data(), X.rows.p, sizeof(int4) * n_rows, hipMemcpyDeviceToHost, st));
  PLACECHECK(hipStreamSynchronize(st));
  X.idle = true;
  const int4* rows = reinterpret_cast<const int4*>(db->stage.data());
  const double step = kTwoPi / (double)S;
  for (int q = 0; q < n_q; ++q) {
    int found = 0;
    for (int k = 0; k < top; ++k) {
      const int4 r = rows[(size_t)q * top + k];
      const double score = r.w > 0 ? (double)r.z / (double)r.w : 0.0;
      if (!(score >= min_score)) break;  // (the rows descend: nothing behind this one passes)
      sicp_place_candidate& o = out[(size_t)q * top_k + found++];
      o.id = first + r.x;
      o.shift = r.y;
      o.match = r.z;
      o.either = r.w;
      o.score = score;
      o.yaw = (double)(2 * r.y > S ? r.y - S : r.y) * step;
    }
    n_found[q] = found;
  }
  return SICP_OK;
}

int check_query(int32_t top_k, double min_score, const void* out, const void* n_found, std::string& why) {
  if (!out) { why = "out is NULL"; return SICP_ERR_INVALID_ARGUMENT; }
  if (!n_found) { why = "n_found is NULL"; return SICP_ERR_INVALID_ARGUMENT; }
  if (top_k < 1) { why = "top_k must be >= 1"; return SICP_ERR_INVALID_ARGUMENT; }
  if (std::isnan(min_score)) { why = "min_score is NaN"; return SICP_ERR_INVALID_ARGUMENT; }
  return SICP_OK;
}

}  // namespace

void place_default_params(sicp_place_params* p) {
  std::memset(p, 0, sizeof *p);
  p->n_rings = 20;
  p->n_sectors = 60;
  p->max_range = 40.0;
  p->channel = SICP_PLACE_LABEL;
  p->z_min = -2.0;
  p->z_step = 0.5;
  p->min_cell_points = 1;
}

int place_create(int device_id, const sicp_place_params* p, sicp_place_ctx** out) {
  if (!out) return SICP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!p || !params_ok(*p)) return SICP_ERR_INVALID_ARGUMENT;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SICP_ERR_NO_DEVICE;
  if (device_id < 0 || device_id >= n) return SICP_ERR_INVALID_ARGUMENT;
  sicp_place_ctx* db = new (std::nothrow) sicp_place_ctx();
  if (!db) return SICP_ERR_OUT_OF_MEMORY;
  db->device = device_id;
  db->params = *p;
  if (p->channel == SICP_PLACE_HEIGHT) {  // (ignored there: kept at zero)
    db->params.num_classes = 0;
    db->params.n_ignore = 0;
  }
  for (int j = std::max(db->params.n_ignore, 0); j < SICP_PLACE_MAX_IGNORE; ++j) db->params.ignore[j] = 0;
  const int R = p->n_rings, S = p->n_sectors;
  db->rs = R * S;
  // rule 2: in double, with libm
  db->tables.resize((size_t)(R + 1 + S));
  double* edge2 = db->tables.data();
  double* cos_half = edge2 + R + 1;
  double* sin_half = cos_half + S / 2;
  const double ring_step = p->max_range / (double)R, sector_step = kTwoPi / (double)S;
  for (int i = 0; i <= R; ++i) {
    const double b = (double)i * ring_step;
    edge2[i] = b * b;
  }
  for (int j = 0; j < S / 2; ++j) {
    const double a = (double)j * sector_step;
    cos_half[j] = std::cos(a);
    sin_half[j] = std::sin(a);
  }
  if (hipSetDevice(device_id) != hipSuccess || db->stream.create() != hipSuccess) {
    delete db;
    return SICP_ERR_NO_DEVICE;
  }
  hipError_t e = db->d_tables.reserve(db->tables.size());
  if (e == hipSuccess) e = hipMemcpyAsync(db->d_tables.p, db->tables.data(), sizeof(double) * db->tables.size(), hipMemcpyHostToDevice, db->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
  if (e != hipSuccess) {
    place_destroy(db);
    return e == hipErrorOutOfMemory ? SICP_ERR_OUT_OF_MEMORY : SICP_ERR_HIP;
  }
  *out = db;
  return SICP_OK;
}

int place_destroy(sicp_place_ctx* db) {
  if (!db) return SICP_OK;
  (void)hipSetDevice(db->device);
  if (db->stream) (void)hipStreamSynchronize(db->stream);
  {
    DevArena::FreeScope once(db->device);  // one wait for the device, not one per buffer
    delete db;
  }
  return SICP_OK;
}

int place_describe(sicp_place_ctx* db, sicp_context* h, int which, const double* sensor_origin, uint8_t* desc, sicp_place_describe_info* info) {
  if (!db) return SICP_ERR_INVALID_ARGUMENT;
  db->call = "sicp_place_describe";
  std::string why;
  if (check_slot(db, h, which, sensor_origin, why) != SICP_OK) {
    db->last_error = "sicp_place_describe: " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  }
  const double t_begin = now_ms();
  sicp_place_describe_info I;
  const int rc = describe_device(db, "sicp_place_describe", h, which, sensor_origin, I);
  if (rc != SICP_OK) return rc;
  if (desc) std::memcpy(desc, staged_desc(db), (size_t)db->rs);
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

int place_add(sicp_place_ctx* db, sicp_context* h, int which, const double* sensor_origin, int32_t* id, uint8_t* desc,
              sicp_place_describe_info* info) {
  if (!db) return SICP_ERR_INVALID_ARGUMENT;
  db->call = "sicp_place_add";
  auto refuse = [&](const std::string& why) {
    db->last_error = "sicp_place_add: " + why + "; the database is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  std::string why;
  if (check_slot(db, h, which, sensor_origin, why) != SICP_OK) return refuse(why);
  if (!id) return refuse("id is NULL");
  if (db->n_entries + 1 > 0x7fffffffll) return refuse("the database would hold more than 2^31 - 1 entries");
  const double t_begin = now_ms();
  sicp_place_describe_info I;
  int rc = describe_device(db, "sicp_place_add", h, which, sensor_origin, I);
  if (rc != SICP_OK) return rc;
  rc = grow_for(db, 1);
  if (rc != SICP_OK) return rc;
  const size_t rs = (size_t)db->rs;
  PLACECHECK(hipMemcpyAsync(db->store[db->cur].p + (size_t)db->n_entries * rs, db->qdesc.p, rs, hipMemcpyDeviceToDevice, db->stream));
  PLACECHECK(hipStreamSynchronize(db->stream));
  *id = (int32_t)db->n_entries;
  db->n_entries += 1;
  if (desc) std::memcpy(desc, staged_desc(db), rs);
  I.t_total_ms = now_ms() - t_begin;
  if (info) *info = I;
  return SICP_OK;
}

int place_add_descriptors(sicp_place_ctx* db, int32_t n, const uint8_t* desc, int32_t* first_id) {
  if (!db) return SICP_ERR_INVALID_ARGUMENT;
  db->call = "sicp_place_add_descriptors";
  auto refuse = [&](const std::string& why) {
    db->last_error = "sicp_place_add_descriptors: " + why + "; the database is unchanged";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  if (n < 1) return refuse("n must be >= 1");
  if (!desc) return refuse("desc is NULL");
  if (db->n_entries + (long long)n > 0x7fffffffll) return refuse("the database would hold more than 2^31 - 1 entries");
  const size_t rs = (size_t)db->rs, bytes = (size_t)n * rs;
  const long long bad = first_bad_byte(db, desc, bytes);
  if (bad >= 0) return refuse(bad_byte_text(db, desc, bad));
  PLACECHECK(hipSetDevice(db->device));
  const int rc = grow_for(db, n);
  if (rc != SICP_OK) return rc;
  PLACECHECK(hipMemcpyAsync(db->store[db->cur].p + (size_t)db->n_entries * rs, desc, bytes, hipMemcpyHostToDevice, db->stream));
  PLACECHECK(hipStreamSynchronize(db->stream));
  if (first_id) *first_id = (int32_t)db->n_entries;
  db->n_entries += n;
  return SICP_OK;
}

int place_get(sicp_place_ctx* db, int32_t first, int32_t count, uint8_t* desc) {
  if (!db) return SICP_ERR_INVALID_ARGUMENT;
  db->call = "sicp_place_get";
  auto refuse = [&](const std::string& why) {
    db->last_error = "sicp_place_get: " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  std::string why;
  if (resolve_range(db, first, count, why) != SICP_OK) return refuse(why);
  if (count == 0) return SICP_OK;
  if (!desc) return refuse("desc is NULL");
  const size_t rs = (size_t)db->rs;
  PLACECHECK(hipSetDevice(db->device));
  PLACECHECK(hipMemcpyAsync(desc, db->store[db->cur].p + (size_t)first * rs, (size_t)count * rs, hipMemcpyDeviceToHost, db->stream));
  PLACECHECK(hipStreamSynchronize(db->stream));
  return SICP_OK;
}

int place_query(sicp_place_ctx* db, sicp_context* h, int which, const double* sensor_origin, int32_t first, int32_t count, int32_t top_k,
                double min_score, sicp_place_candidate* out, int32_t* n_found) {
  if (!db) return SICP_ERR_INVALID_ARGUMENT;
  db->call = "sicp_place_query";
  auto refuse = [&](const std::string& why) {
    db->last_error = "sicp_place_query: " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  std::string why;
  if (check_slot(db, h, which, sensor_origin, why) != SICP_OK) return refuse(why);
  if (check_query(top_k, min_score, out, n_found, why) != SICP_OK) return refuse(why);
  if (resolve_range(db, first, count, why) != SICP_OK) return refuse(why);
  sicp_place_describe_info I;
  const int rc = describe_device(db, "sicp_place_query", h, which, sensor_origin, I);
  if (rc != SICP_OK) return rc;
  return search_device(db, 1, first, count, top_k, min_score, out, n_found);
}

int place_query_descriptors(sicp_place_ctx* db, int32_t n_q, const uint8_t* desc, int32_t first, int32_t count, int32_t top_k,
                            double min_score, sicp_place_candidate* out, int32_t* n_found) {
  if (!db) return SICP_ERR_INVALID_ARGUMENT;
  db->call = "sicp_place_query_descriptors";
  auto refuse = [&](const std::string& why) {
    db->last_error = "sicp_place_query_descriptors: " + why + "; nothing was written";
    return SICP_ERR_INVALID_ARGUMENT;
  };
  std::string why;
  if (n_q < 1) return refuse("n_q must be >= 1");
  if (!desc) return refuse("desc is NULL");
  if (check_query(top_k, min_score, out, n_found, why) != SICP_OK) return refuse(why);
  if (resolve_range(db, first, count, why) != SICP_OK) return refuse(why);
  if ((long long)n_q * (long long)count > 0x7fffffffll) return refuse("n_q * count exceeds 2^31 - 1 (query, entry) pairs: split the batch");
  const size_t bytes = (size_t)n_q * (size_t)db->rs;
  const long long bad = first_bad_byte(db, desc, bytes);
  if (bad >= 0) return refuse(bad_byte_text(db, desc, bad));
  PLACECHECK(hipSetDevice(db->device));
  if (count > 0) {
    PLACECHECK(db->qdesc.reserve(bytes));
    PLACECHECK(hipMemcpyAsync(db->qdesc.p, desc, bytes, hipMemcpyHostToDevice, db->stream));
    PLACECHECK(hipStreamSynchronize(db->stream));
  }
  return search_device(db, n_q, first, count, top_k, min_score, out, n_found);
}

int place_tables(sicp_place_ctx* db, double* cos_half, double* sin_half, double* edge2) {
  if (!db) return SICP_ERR_INVALID_ARGUMENT;
  const int R = db->params.n_rings, S = db->params.n_sectors;
  const double* t = db->tables.data();
  if (edge2) std::memcpy(edge2, t, sizeof(double) * (size_t)(R + 1));
  if (cos_half) std::memcpy(cos_half, t + R + 1, sizeof(double) * (size_t)(S / 2));
  if (sin_half) std::memcpy(sin_half, t + R + 1 + S / 2, sizeof(double) * (size_t)(S / 2));
  return SICP_OK;
}

}  // namespace host
}  // namespace sicp
