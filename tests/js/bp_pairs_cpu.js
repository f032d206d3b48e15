'use strict';
/* CPU-side checks of the JavaScript layer of the back-projection over pairs (driven by tests/test_bp_pairs_cpu.py; no GPU):
 *     node tests/js/bp_pairs_cpu.js job.json
 *  1. tests/js/bp_pairs_common.js on tests/js/mock_addon_bp_pairs.js with the entry point present: MultiTracker's getters equal M
 *     camshift.Tracker instances and the reference's recorded CRCs / samples, one (counted) device call per getBackProjectionImgs();
 *  2. the same with the entry point absent (withBpPairs(false)): the host loop, no device call, same results;
 *  3. ccv.DeviceBatch.backProjectionPairs on mixed feeds — both sequences as the two feeds of a batch, a shuffled subset of the trackers
 *     per call — against the recorded CRCs and samples; its argument errors; an addon without the entry point is named in the Error.
 * Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const mock = require(path.join(__dirname, 'mock_addon_bp_pairs.js'));
mock.install();
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));
const common = require(path.join(__dirname, 'bp_pairs_common.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], imgs_calls: 0, crc_checks: 0, pdf_checks: 0, single_checks: 0, batch_checks: 0, missing_checks: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const counters = function () { return mock.calls.camshiftBackProjectPairs || 0; };

common(headtrackr, Canvas, job, out, check, counters, { full: true, device: true });
out.device_calls_present = counters();
mock.withBpPairs(false);
common(headtrackr, Canvas, job, out, check, counters, { full: true, device: false });
out.device_calls_absent = counters() - out.device_calls_present;

/* 3. DeviceBatch.backProjectionPairs */
{
  const A = job.cases[0], B = job.cases[1], w = A.w, h = A.h, npix = w * h;
  check(B.w === w && B.h === h && A.frames.length === B.frames.length, 'both sequences have one size and length');
  const trackers = []; /* [feed, tracker of the feed, slot] */
  const slotsOf = [6, 2, 9, 0, 5];
  A.rects.forEach(function (_r, j) { trackers.push([0, j, slotsOf[trackers.length]]); });
  B.rects.forEach(function (_r, j) { trackers.push([1, j, slotsOf[trackers.length]]); });
  const b = new headtrackr.ccv.DeviceBatch(w, h, 2, { depth: 1, sets: A.frames.length, trackers: 10 });
  A.frames.forEach(function (f, k) {
    const set = new Uint8Array(8 * npix);
    set.set(fs.readFileSync(f), 0); set.set(fs.readFileSync(B.frames[k]), 4 * npix);
    b.upload(set, k);
  });
  mock.withBpPairs(true);
  let threw = false;
  try { b.backProjectionPairs(0, new Int32Array([0, 0]), 'rgba8'); } catch (e) { threw = /no trackers/.test(e.message); }
  check(threw, 'backProjectionPairs before any tracker exists must throw');
  const ip = new Int32Array(2 * trackers.length), rc = new Int32Array(4 * trackers.length);
  trackers.forEach(function (t, i) { ip[2 * i] = t[2]; ip[2 * i + 1] = t[0]; rc.set((t[0] ? B : A).rects[t[1]], 4 * i); });
  b.initPairs(0, ip, rc);
  threw = false;
  try { b.backProjectionPairs(1, ip, 'f32'); } catch (e) { threw = e instanceof RangeError; }
  check(threw, 'an unknown kind is a RangeError');
  threw = false;
  try { b.backProjectionPairs(1, [0, 0], 'rgba8'); } catch (e) { threw = e instanceof TypeError; }
  check(threw, 'pairs that are no Int32Array are a TypeError');
  threw = false;
  try { b.backProjectionPairs(1, new Int32Array([6, 0, 6, 1]), 'rgba8'); } catch (e) { threw = /status -1/.test(e.message); }
  check(threw, 'a stream named twice is refused with status -1');
  /* feeds in different states: call k projects a different subset of the trackers, in another order */
  const subsets = [[4, 0, 2], [1, 3], [2, 4, 1, 0, 3], [3]];
  for (let k = 1; k < A.frames.length; k++) {
    const sub = subsets[(k - 1) % subsets.length], pr = new Int32Array(2 * sub.length);
    sub.forEach(function (t, i) { pr[2 * i] = trackers[t][2]; pr[2 * i + 1] = trackers[t][0]; });
    const rgba = b.backProjectionPairs(k, pr, 'rgba8'), pdf = b.backProjectionPairs(k, pr, 'f64');
    check(rgba instanceof Uint8Array && rgba.length === 4 * sub.length * npix && pdf instanceof Float64Array && pdf.length === sub.length * npix, 'set ' + k + ': result shapes');
    sub.forEach(function (t, i) {
      const rec = (trackers[t][0] ? B : A).trackers[trackers[t][1]][k - 1];
      let ok = check(common.crc32(rgba.subarray(4 * npix * i, 4 * npix * (i + 1))) === rec.crc, 'set ' + k + ' pair ' + i + ': CRC');
      rec.pdf.forEach(function (s) { ok = check(Object.is(pdf[i * npix + s[1] * w + s[0]], s[2]), 'set ' + k + ' pair ' + i + ': pdf sample') && ok; });
      if (ok) out.batch_checks++;
    });
  }
  /* the trackers are untouched: a pair track step after the back-projections equals one on a fresh batch */
  const t1 = b.trackPairs(1, ip, true);
  mock.withBpPairs(false);
  threw = false;
  const before = JSON.stringify(mock.calls);
  try { b.backProjectionPairs(1, ip, 'rgba8'); } catch (e) { threw = /camshiftBackProjectPairs/.test(e.message); }
  if (check(threw && JSON.stringify(mock.calls) === before, 'backProjectionPairs on an addon without the entry point must throw before it reaches the addon')) out.missing_checks++;
  b.destroy();
  const b2 = new headtrackr.ccv.DeviceBatch(w, h, 2, { depth: 1, sets: 2, trackers: 10 });
  [0, 1].forEach(function (k) {
    const set = new Uint8Array(8 * npix);
    set.set(fs.readFileSync(A.frames[k]), 0); set.set(fs.readFileSync(B.frames[k]), 4 * npix);
    b2.upload(set, k);
  });
  b2.initPairs(0, ip, rc);
  const t2 = b2.trackPairs(1, ip, true);
  let same = t1.length === t2.length;
  for (let i = 0; same && i < t1.length; i++) same = Object.is(t1[i], t2[i]);
  check(same, 'pair track step after back-projections == pair track step without');
  b2.destroy();
  mock.withBpPairs(true);
}

process.stdout.write(JSON.stringify(out) + '\n');
