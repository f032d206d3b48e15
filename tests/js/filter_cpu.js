'use strict';
/* CPU-side checks of opts.prefilter in ccv.DeviceBatch's cropPairs / cropFeeds / alignPairs / alignFeeds (driven by tests/test_filter_cpu.py;
 * no GPU):   node tests/js/filter_cpu.js job.json
 * job: tests/js/patch_cpu.js's, with `prefilters`: [1..8, ...] and ONE config.  For the pairs form and the feeds form, for crop and align:
 * first the call without opts.prefilter (its result must be what it always was, through the entry point it always took), then one call per
 * prefilter, then prefilter[0] together with tensors[0], then the plain call again; the CRC-32 of the patches' bytes, their typed-array kind,
 * the `factors` and the entry points that were called are printed, Python compares them with the restatement.  Malformed opts.prefilter
 * throw; an addon without the filtered calls gives the rebuild-it error.  One JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_filter.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], pairs: { crop: [], align: [] }, feeds: { crop: [], align: [] }, refusals: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const CRC = (function () { const t = new Int32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); t[n] = c; } return t; })();
function crc32(buf) { let c = -1; for (let i = 0; i < buf.length; i++) c = CRC[(c ^ buf[i]) & 0xFF] ^ (c >>> 8); return (c ^ -1) >>> 0; }
function throwsLike(fn, re, what) { let ok = false; try { fn(); } catch (e) { ok = re.test(e.message); if (!ok) out.errors.push(what + ': threw "' + e.message + '"'); } if (check(ok, what)) out.refusals++; }
const ENTRY = /^(crop|align)(Pairs|Sources)(Tensor|Filtered)?Device$/;
function entryCalls() { const c = {}; Object.keys(mock.calls).forEach(function (k) { if (ENTRY.test(k) && mock.calls[k]) c[k] = mock.calls[k]; }); return c; }
function report(r, before) {
  const bytes = new Uint8Array(r.patches.buffer, r.patches.byteOffset, r.patches.byteLength), now = entryCalls(), called = [];
  Object.keys(now).forEach(function (k) { for (let i = before[k] || 0; i < now[k]; i++) called.push(k); });
  return { n: r.n, size: [r.width, r.height], kind: r.patches.constructor.name, length: r.patches.length, crc: crc32(bytes), records: Array.from(r.records),
           extra: Array.from(r.ratios || r.terms), tensor: r.tensor === undefined ? null : r.tensor, factors: r.factors === undefined ? null : Array.from(r.factors), called: called };
}
mock.withIngest(true); mock.withYuv(true); mock.withDrawList(true); mock.withCrop(true); mock.withAlign(true); mock.withPatch(true); mock.withFilter(true);
const cfg = job.configs[0];
function all(call, result, dst) {
  const run = function (o) { const before = entryCalls(); call(o); dst.push(report(result(), before)); };
  run(cfg);
  job.prefilters.forEach(function (p) { run(Object.assign({ prefilter: p }, cfg)); });
  run(Object.assign({ prefilter: job.prefilters[0], tensor: job.tensors[0] }, cfg));
  run(cfg);  /* and the plain call again behind the filtered calls: nothing sticks */
}

(function () {
  const p = job.pairs, pairs = Int32Array.from(p.align_pairs);
  const db = new headtrackr.ccv.DeviceBatch(job.w, job.h, 2, { depth: 1, sets: 2, trackers: p.trackers });
  db.upload(new Uint8Array(fs.readFileSync(p.init)), 0);
  db.upload(new Uint8Array(fs.readFileSync(p.step)), 1);
  db.initPairs(0, Int32Array.from(p.init_pairs), Int32Array.from(p.rects));
  db.trackPairs(1, Int32Array.from(p.track_pairs), true);
  all(function (o) { db.cropPairs(1, pairs, o); }, function () { return db.cropResult(); }, out.pairs.crop);
  all(function (o) { db.alignPairs(1, pairs, o); }, function () { return db.alignResult(); }, out.pairs.align);
  ['cropPairs', 'alignPairs'].forEach(function (m) {
    [0, 9, -1, 2.5, '8', true].forEach(function (bad) {
      throwsLike(function () { db[m](1, pairs, Object.assign({}, cfg, { prefilter: bad })); }, /opts\.prefilter is an integer 1\.\.8/, m + ': prefilter ' + JSON.stringify(bad) + ' throws');
    });
  });
  mock.withFilter(false);
  throwsLike(function () { db.cropPairs(1, pairs, Object.assign({ prefilter: 8 }, cfg)); }, /no cropPairsFilteredDevice \/ cropFilterFactors \(rebuild it\)/, 'an addon without the filtered calls gives the rebuild-it error');
  db.cropPairs(1, pairs, Object.assign({ tensor: job.tensors[0] }, cfg));  /* ... and serves tensors and RGBA as before */
  check(db.cropResult().factors === undefined, 'without opts.prefilter the result has no factors');
  mock.withFilter(true);
  db.destroy();
})();

(function () {
  const f = job.feeds, n = f.list.length;
  const sources = f.list.map(function (e) { const s = { width: e.width, height: e.height, format: e.format }; if (e.format !== 'rgba') s.matrix = e.matrix; return s; });
  const rects = f.list.map(function (e) { return e.rect; });
  const db = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 1, sets: 1, sources: sources, trackers: f.trackers });
  f.list.forEach(function (e, i) { db.uploadSourceOf(i, new Uint8Array(fs.readFileSync(e.file))); });
  db.drawList(0, 0, rects);
  const pairs = new Int32Array(2 * n), init = new Int32Array(4 * n);
  f.list.forEach(function (e, i) { pairs[2 * i] = f.streams[i]; pairs[2 * i + 1] = i; init.set(e.init, 4 * i); });
  db.initPairs(0, pairs, init);
  db.trackPairs(0, pairs, true);
  const streams = Int32Array.from(f.streams);
  all(function (o) { db.cropFeeds(0, streams, Object.assign({ rects: rects }, o)); }, function () { return db.cropResult(); }, out.feeds.crop);
  all(function (o) { db.alignFeeds(0, streams, Object.assign({ rects: rects }, o)); }, function () { return db.alignResult(); }, out.feeds.align);
  throwsLike(function () { db.cropFeeds(0, streams, Object.assign({ rects: rects, prefilter: 0 }, cfg)); }, /opts\.prefilter/, 'cropFeeds: prefilter 0 throws');
  throwsLike(function () { db.alignFeeds(0, streams, Object.assign({ rects: rects, prefilter: 9 }, cfg)); }, /opts\.prefilter/, 'alignFeeds: prefilter 9 throws');
  db.destroy();
})();

process.stdout.write(JSON.stringify(out) + '\n');
