'use strict';
/* CPU-side checks of the aligned crops' JavaScript layer (driven by tests/test_align_cpu.py; no GPU):
 *     node tests/js/align_cpu.js job.json
 * job: { w, h, configs: [{width, height, margin, square}],
 *        pairs: {init (file: 2 frames), step (file: 2 frames), trackers, init_pairs, rects, track_pairs, align_pairs},
 *        feeds: {list: [{file, width, height, format, matrix, rect | null, init: [x, y, w, h]}], streams, trackers} }
 *  1. ccv.DeviceBatch: initPairs, an ENQUEUE-ONLY track step, then alignPairs per config and alignResult: the CRC-32 of every patch, the records
 *     and the terms are printed, Python compares them with the numpy / oracle expectation; only then is the track step collected;
 *  2. a batch with mixed opts.sources: uploadSourceOf, drawList under the rects, initPairs + trackPairs on the drawn canvases, alignFeeds per
 *     config with the same rects;
 *  3. malformed calls throw; an addon without the align calls gives the "rebuild it" error.
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_align.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], pairs: [], feeds: [], refusals: 0, track: null };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const CRC = (function () { const t = new Int32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); t[n] = c; } return t; })();
function crc32(buf) { let c = -1; for (let i = 0; i < buf.length; i++) c = CRC[(c ^ buf[i]) & 0xFF] ^ (c >>> 8); return (c ^ -1) >>> 0; }
function calls(k) { return mock.calls[k] || 0; }
function throwsLike(fn, re, what) { let ok = false; try { fn(); } catch (e) { ok = re.test(e.message); if (!ok) out.errors.push(what + ': threw "' + e.message + '"'); } if (check(ok, what)) out.refusals++; }
function report(r) {
  const pb = r.width * r.height * 4, crc = [];
  for (let i = 0; i < r.n; i++) crc.push(crc32(r.patches.subarray(i * pb, (i + 1) * pb)));
  return { n: r.n, size: [r.width, r.height], crc: crc, records: Array.from(r.records), terms: Array.from(r.terms), bytes: r.patches.length };
}
mock.withIngest(true); mock.withYuv(true); mock.withDrawList(true); mock.withCrop(true); mock.withAlign(true);

/* 1. the pairs form behind an enqueue-only track step */
(function () {
  const p = job.pairs;
  const db = new headtrackr.ccv.DeviceBatch(job.w, job.h, 2, { depth: 1, sets: 2, trackers: p.trackers });
  throwsLike(function () { db.alignPairs(0, Int32Array.from(p.align_pairs), job.configs[0]); }, /no trackers yet/, 'alignPairs before any tracker throws');
  throwsLike(function () { db.alignResult(); }, /no alignPairs/, 'alignResult before any align call throws');
  db.upload(new Uint8Array(fs.readFileSync(p.init)), 0);
  db.upload(new Uint8Array(fs.readFileSync(p.step)), 1);
  db.initPairs(0, Int32Array.from(p.init_pairs), Int32Array.from(p.rects));
  db.trackPairsEnqueue(1, Int32Array.from(p.track_pairs), true);
  const before = calls('alignPairsDevice');
  job.configs.forEach(function (cfg) { db.alignPairs(1, Int32Array.from(p.align_pairs), cfg); out.pairs.push(report(db.alignResult())); });
  check(calls('alignPairsDevice') === before + job.configs.length && calls('drawFramesDevice') === 0, 'the facade must take alignPairsDevice, one call per alignPairs');
  out.track = Array.from(db.trackCollect());
  const good = job.configs[0], pairs = Int32Array.from(p.align_pairs);
  throwsLike(function () { db.alignPairs(1, pairs); }, /opts is/, 'alignPairs without opts throws');
  throwsLike(function () { db.alignPairs(1, Array.from(pairs), good); }, /pairs is an Int32Array/, 'pairs as a plain array throws');
  throwsLike(function () { db.alignPairs(1, pairs, Object.assign({}, good, { width: 0 })); }, /1\.\.1024/, 'width 0 throws');
  throwsLike(function () { db.alignPairs(1, pairs, Object.assign({}, good, { height: 1025 })); }, /1\.\.1024/, 'height 1025 throws');
  throwsLike(function () { db.alignPairs(1, pairs, Object.assign({}, good, { width: 7.5 })); }, /1\.\.1024/, 'a fractional width throws');
  throwsLike(function () { db.alignPairs(1, pairs, Object.assign({}, good, { margin: 0.2 })); }, /margin/, 'margin 0.2 throws');
  throwsLike(function () { db.alignPairs(1, pairs, Object.assign({}, good, { margin: 4.01 })); }, /margin/, 'margin 4.01 throws');
  throwsLike(function () { db.alignPairs(1, pairs, Object.assign({}, good, { margin: 'wide' })); }, /margin/, 'a margin that is no number throws');
  throwsLike(function () { db.alignPairs(1, Int32Array.from([p.trackers, 0]), good); }, /not reserved/, 'an unreserved tracker is refused by the addon');
  throwsLike(function () { db.alignPairs(1, Int32Array.from([0, 2]), good); }, /entry 0/, 'an unbound frame is refused by the addon, naming the entry');
  throwsLike(function () { db.alignFeeds(0, Int32Array.from([0, 1]), good); }, /opts\.sources/, 'alignFeeds on a batch without opts.sources throws');
  mock.withAlign(false);
  throwsLike(function () { db.alignPairs(1, pairs, good); }, /no alignPairsDevice .* \(rebuild it\)/, 'an addon without the align calls gives the rebuild-it error');
  mock.withAlign(true);
  db.destroy();
})();

/* 2. the sources form on mixed feeds */
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
  const before = calls('alignSourcesDevice'), streams = Int32Array.from(f.streams);
  job.configs.forEach(function (cfg) { db.alignFeeds(0, streams, Object.assign({ rects: rects }, cfg)); out.feeds.push(report(db.alignResult())); });
  check(calls('alignSourcesDevice') === before + job.configs.length, 'the facade must take alignSourcesDevice, one call per alignFeeds');
  const good = Object.assign({ rects: rects }, job.configs[0]);
  throwsLike(function () { db.alignFeeds(0, streams.subarray(1), good); }, /one tracker per feed/, 'a streams list of the wrong length throws');
  throwsLike(function () { db.alignFeeds(0, Array.from(streams), good); }, /one tracker per feed/, 'streams as a plain array throws');
  throwsLike(function () { db.alignFeeds(0, streams, Object.assign({}, good, { rects: rects.slice(1) })); }, /rects is null or an array/, 'a rects array of the wrong length throws');
  throwsLike(function () { db.alignFeeds(1, streams, good); }, /source set/, 'a source set the feeds do not have throws');
  throwsLike(function () { db.alignFeeds(0, streams, Object.assign({}, good, { rects: rects.map(function (r, i) { return i === 1 ? [0, 0, f.list[1].width + 1, 1] : r; }) })); }, /entry 1/, 'a rect outside its source is refused by the addon, naming the entry');
  db.destroy();
})();

process.stdout.write(JSON.stringify(out) + '\n');
