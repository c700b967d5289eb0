// jb_huff_pack.cpp -- packing of device-entropy submissions (see jb_huff.h): sizes derived from untrusted files turned
// into offsets and memcpys.  Pure host code, no HIP: the batch decoder's threads, tools/fuzz (under the sanitizers) and
// tools/huff_emu run exactly this.
#include <cstring>
#include <vector>

#include "jb_huff.h"

size_t jb_huff_pack_size_(const JbHuffJob *const *jobs, int n) {
  size_t n_wg = 0, n_starts = 0, scan_bytes = 0, n_chunks = 0;
  for (int i = 0; i < n; i++) {
    n_wg += (jobs[i]->img.n_chunks + kJbOwnChunks - 1) / kJbOwnChunks;
    n_chunks += jobs[i]->img.n_chunks;
    n_starts += jobs[i]->starts.size();
    scan_bytes += ((jobs[i]->scan.size() + 15) & ~(size_t)15);
  }
  // (every workgroup twice: the list of all of them and the list of the ones that synchronise)
  return (size_t)n * sizeof(JbHuffImage) + 2 * n_wg * sizeof(JbHuffWg) + (size_t)n * sizeof(JbHuffTables) + n_starts * 4 +
         n_chunks * sizeof(JbChunkDesc) + scan_bytes + 512;
}

int jb_huff_pack_(const JbHuffJob *const *jobs, int n, int64_t coef_stride, uint8_t *h, JbHuffLayout *lay) {
  auto a16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  std::vector<int> set_of((size_t)n, 0);
  std::vector<int> sets;  // index of the first job that owns each distinct table set
  size_t n_wg = 0, n_sync_wg = 0, n_starts = 0, scan_bytes = 0, n_chunks = 0;
  lay->max_chunk_bytes = 0;
  lay->max_tabs = 0;
  for (int i = 0; i < n; i++) {
    int found = -1;
    for (size_t k = 0; k < sets.size() && found < 0; k++)
      if (jobs[sets[k]]->n_tabs == jobs[i]->n_tabs && memcmp(&jobs[sets[k]]->tables, &jobs[i]->tables, sizeof(JbHuffTables)) == 0) found = (int)k;
    if (found < 0) {
      found = (int)sets.size();
      sets.push_back(i);
    }
    set_of[(size_t)i] = found;
    const size_t wgs = (jobs[i]->img.n_chunks + kJbOwnChunks - 1) / kJbOwnChunks;
    n_wg += wgs;
    if (jobs[i]->img.needs_sync) n_sync_wg += wgs;
    n_chunks += jobs[i]->img.n_chunks;
    n_starts += jobs[i]->starts.size();
    scan_bytes += a16(jobs[i]->scan.size());
    if (jobs[i]->img.chunk_bytes > lay->max_chunk_bytes) lay->max_chunk_bytes = jobs[i]->img.chunk_bytes;
    if (jobs[i]->n_tabs > lay->max_tabs) lay->max_tabs = jobs[i]->n_tabs;
    // (a frame that changed between the passes of a batch decoder must not write beyond its slot)
    if ((int64_t)jobs[i]->geo.coef_bytes > coef_stride) return JB_ERR_CAPACITY;
  }
  lay->off_img = 0;
  lay->off_wg = a16((size_t)n * sizeof(JbHuffImage));
  lay->off_sync_wg = a16(lay->off_wg + n_wg * sizeof(JbHuffWg));
  lay->off_tab = a16(lay->off_sync_wg + n_sync_wg * sizeof(JbHuffWg));
  lay->off_starts = lay->off_tab + sets.size() * sizeof(JbHuffTables);
  lay->off_chunks = a16(lay->off_starts + n_starts * 4);
  lay->off_scan = a16(lay->off_chunks + n_chunks * sizeof(JbChunkDesc));
  lay->total = lay->off_scan + scan_bytes + 256;  // (a lane reads up to 16 dwords beyond its chunk's last byte)
  // device-only scratch behind the uploaded bytes
  lay->off_entry = a16(lay->total);
  lay->off_exit = a16(lay->off_entry + n_chunks * sizeof(JbChunkState));
  lay->off_cps = a16(lay->off_exit + n_chunks * sizeof(JbChunkState));
  lay->off_chunk_dc = (a16(lay->off_cps + n_chunks * kJbCheckpoints * 4) + 31) & ~(size_t)31;
  lay->off_wgsum = lay->off_chunk_dc + n_chunks * sizeof(JbChunkDc);
  lay->device_total = a16(lay->off_wgsum + n_wg * sizeof(JbWgSum));
  lay->n = n;
  lay->n_wg = (int)n_wg;
  lay->n_sync_wg = (int)n_sync_wg;
  lay->n_chunks = (uint32_t)n_chunks;
  lay->coef_stride = coef_stride;
  if (lay->device_total > 0xffffff00u || n_wg > 0x7fffffffu || n_chunks > 0x3fffffffu) return JB_ERR_CAPACITY;
  JbHuffImage *im = (JbHuffImage *)(h + lay->off_img);
  JbHuffWg *wg = (JbHuffWg *)(h + lay->off_wg);
  JbHuffWg *swg = (JbHuffWg *)(h + lay->off_sync_wg);
  uint32_t *st = (uint32_t *)(h + lay->off_starts);
  size_t w = 0, sw = 0, si = 0, sc = lay->off_scan, chunk0 = 0;
  for (size_t k = 0; k < sets.size(); k++) memcpy(h + lay->off_tab + k * sizeof(JbHuffTables), &jobs[sets[k]]->tables, sizeof(JbHuffTables));
  for (int i = 0; i < n; i++) {
    const JbHuffJob &j = *jobs[i];
    im[i] = j.img;
    im[i].scan_off = (uint32_t)(sc - lay->off_scan);
    im[i].int_off = (uint32_t)si;
    im[i].table_set = (uint32_t)set_of[(size_t)i];
    im[i].coef_off = (int64_t)i * coef_stride;
    im[i].state_off = (uint32_t)chunk0;
    im[i].wg0 = (uint32_t)w;
    // the chunks of every restart interval, from the interval's first byte (jb_chunks_of_)
    JbChunkDesc *cd = (JbChunkDesc *)(h + lay->off_chunks) + chunk0;
    uint32_t c = 0;
    for (uint32_t seg = 0; seg + 1 < (uint32_t)j.starts.size(); seg++) {
      const uint32_t k = jb_chunks_of_(j.starts[seg + 1] - j.starts[seg], j.img.chunk_bytes);
      if (c + k > j.img.n_chunks) return JB_ERR_STATE;
      for (uint32_t q = 0; q < k; q++) cd[c++] = JbChunkDesc{j.starts[seg] + q * j.img.chunk_bytes, seg | (q == 0 ? 0x80000000u : 0u)};
    }
    if (c != j.img.n_chunks) return JB_ERR_STATE;
    chunk0 += j.img.n_chunks;
    for (uint32_t f = 0; f < j.img.n_chunks; f += kJbOwnChunks) {
      wg[w++] = JbHuffWg{(uint32_t)i, f};
      if (j.img.needs_sync) swg[sw++] = JbHuffWg{(uint32_t)i, f};
    }
    memcpy(st + si, j.starts.data(), j.starts.size() * 4);
    si += j.starts.size();
    memcpy(h + sc, j.scan.data(), j.scan.size());
    sc += a16(j.scan.size());
  }
  memset(h + sc, 0, 256);
  return JB_OK;
}
