'use strict';
/* CPU-side checks of opts.tensor in ccv.DeviceBatch's cropPairs / cropFeeds / alignPairs / alignFeeds (driven by tests/test_patch_tensor_cpu.py;
 * no GPU):   node tests/js/patch_cpu.js job.json
 * job: tests/js/align_cpu.js's, with `tensors`: [{dtype, layout, channels, scale, bias}] and ONE config.  For the pairs form and the feeds
 * form, for crop and align: first the call without opts.tensor (its result must be what it always was: a Uint8Array), then one call per
 * tensor format; the CRC-32 of the patches' bytes, their typed-array kind and length and the `tensor` field are printed, Python compares
 * them with the restatement.  Malformed opts.tensor throw; an addon without the tensor calls gives the rebuild-it error.  One JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_patch.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], pairs: { crop: [], align: [] }, feeds: { crop: [], align: [] }, refusals: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const CRC = (function () { const t = new Int32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); t[n] = c; } return t; })();
function crc32(buf) { let c = -1; for (let i = 0; i < buf.length; i++) c = CRC[(c ^ buf[i]) & 0xFF] ^ (c >>> 8); return (c ^ -1) >>> 0; }
function calls(k) { return mock.calls[k] || 0; }
function throwsLike(fn, re, what) { let ok = false; try { fn(); } catch (e) { ok = re.test(e.message); if (!ok) out.errors.push(what + ': threw "' + e.message + '"'); } if (check(ok, what)) out.refusals++; }
function report(r) {
  const bytes = new Uint8Array(r.patches.buffer, r.patches.byteOffset, r.patches.byteLength);
  return { n: r.n, size: [r.width, r.height], kind: r.patches.constructor.name, length: r.patches.length, crc: crc32(bytes), records: Array.from(r.records),
           extra: Array.from(r.ratios || r.terms), tensor: r.tensor === undefined ? null : r.tensor };
}
mock.withIngest(true); mock.withYuv(true); mock.withDrawList(true); mock.withCrop(true); mock.withAlign(true); mock.withPatch(true);
const cfg = job.configs[0];
function both(db, kind, call, result, dst) {
  call(cfg); dst.push(report(result()));
  job.tensors.forEach(function (t) { call(Object.assign({ tensor: t }, cfg)); dst.push(report(result())); });
  call(cfg); dst.push(report(result()));  /* and RGBA again behind the tensor calls: nothing sticks */
}

(function () {
  const p = job.pairs, pairs = Int32Array.from(p.align_pairs);
  const db = new headtrackr.ccv.DeviceBatch(job.w, job.h, 2, { depth: 1, sets: 2, trackers: p.trackers });
  db.upload(new Uint8Array(fs.readFileSync(p.init)), 0);
  db.upload(new Uint8Array(fs.readFileSync(p.step)), 1);
  db.initPairs(0, Int32Array.from(p.init_pairs), Int32Array.from(p.rects));
  db.trackPairs(1, Int32Array.from(p.track_pairs), true);
  const rgbaBefore = calls('cropPairsDevice') + calls('alignPairsDevice');
  both(db, 'crop', function (o) { db.cropPairs(1, pairs, o); }, function () { return db.cropResult(); }, out.pairs.crop);
  both(db, 'align', function (o) { db.alignPairs(1, pairs, o); }, function () { return db.alignResult(); }, out.pairs.align);
  check(calls('cropPairsTensorDevice') === job.tensors.length && calls('alignPairsTensorDevice') === job.tensors.length, 'one tensor entry point call per call with opts.tensor');
  check(calls('cropPairsDevice') + calls('alignPairsDevice') === rgbaBefore + 4, 'the RGBA entry points are taken only without opts.tensor');
  const good = Object.assign({ tensor: job.tensors[0] }, cfg), T = job.tensors[0];
  const withT = function (t) { return Object.assign({}, cfg, { tensor: Object.assign({}, T, t) }); };
  ['cropPairs', 'alignPairs'].forEach(function (m) {
    throwsLike(function () { db[m](1, pairs, Object.assign({}, cfg, { tensor: 'f16' })); }, /opts\.tensor is/, m + ': a tensor that is no object throws');
    throwsLike(function () { db[m](1, pairs, withT({ dtype: 'f64' })); }, /dtype/, m + ': an unknown dtype throws');
    throwsLike(function () { db[m](1, pairs, withT({ layout: 'nchw' })); }, /layout/, m + ': an unknown layout throws');
    throwsLike(function () { db[m](1, pairs, withT({ channels: 'rgba' })); }, /channels/, m + ': an unknown channels value throws');
    throwsLike(function () { db[m](1, pairs, withT({ scale: [1, 2] })); }, /scale/, m + ': two scales for three channels throw');
    throwsLike(function () { db[m](1, pairs, withT({ bias: ['0', 0, 0] })); }, /bias/, m + ': a bias that is no number throws');
    throwsLike(function () { db[m](1, pairs, withT({ scale: 1e30 })); }, /out of bounds/, m + ': a scale beyond 2^64 is refused by the addon');
  });
  mock.withPatch(false);
  throwsLike(function () { db.cropPairs(1, pairs, good); }, /no cropPairsTensorDevice \(rebuild it\)/, 'an addon without the tensor calls gives the rebuild-it error');
  db.cropPairs(1, pairs, cfg);  /* ... and serves RGBA as before */
  check(db.cropResult().patches instanceof Uint8Array, 'without opts.tensor an addon without the tensor calls still crops');
  mock.withPatch(true);
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
  both(db, 'crop', function (o) { db.cropFeeds(0, streams, Object.assign({ rects: rects }, o)); }, function () { return db.cropResult(); }, out.feeds.crop);
  both(db, 'align', function (o) { db.alignFeeds(0, streams, Object.assign({ rects: rects }, o)); }, function () { return db.alignResult(); }, out.feeds.align);
  check(calls('cropSourcesTensorDevice') === job.tensors.length && calls('alignSourcesTensorDevice') === job.tensors.length, 'one sources tensor entry point call per cropFeeds / alignFeeds with opts.tensor');
  db.destroy();
})();

process.stdout.write(JSON.stringify(out) + '\n');
