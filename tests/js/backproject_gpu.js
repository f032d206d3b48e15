'use strict';
/* The device back-projection from the JavaScript host, on a GPU (driven by tests/test_gpu_backproject.py):
 *     node tests/js/backproject_gpu.js job.json
 * job: { w, h, n, rects[4n], sets[raw files of n frames], expect[{set, rgba8, f64}] (raw files written from the expectation),
 *        golden[{name, w, h, rect, calcAngles, frames[raw files], calls[frame index per track()], crc}] }
 * ccv.DeviceBatch.backProjection must return the expectation's bytes for every listed set and kind; camshift.Tracker.getBackProjectionImg()
 * must return the reference's CRC-32 for every golden case AND get its bytes from the addon's camshiftBackProject — counted by wrapping the
 * addon's function here, not by a counter in the product.  Prints one JSON line. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const A = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr_hip.node'));
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = { ok: true, errors: [], device_calls: 0, batch_checks: 0, golden_checks: 0 };
function check(cond, msg) { if (!cond) { out.ok = false; if (out.errors.length < 20) out.errors.push(msg); } return cond; }
const CRC = (function () { const t = new Int32Array(256); for (let n = 0; n < 256; n++) { let c = n; for (let k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320 ^ (c >>> 1)) : (c >>> 1); t[n] = c; } return t; })();
function crc32(buf) { let c = -1; for (let i = 0; i < buf.length; i++) c = CRC[(c ^ buf[i]) & 0xFF] ^ (c >>> 8); return (c ^ -1) >>> 0; }
function sameBytes(a, b) { /* typed arrays of any kind, compared byte for byte */
  const x = new Uint8Array(a.buffer, a.byteOffset, a.byteLength), y = new Uint8Array(b.buffer, b.byteOffset, b.byteLength);
  if (x.length !== y.length) return false;
  for (let i = 0; i < x.length; i++) if (x[i] !== y[i]) return false;
  return true;
}

const real = A.camshiftBackProject;
check(typeof real === 'function' && A.BP_RGBA8 === 0 && A.BP_F64 === 1, 'addon exports');
A.camshiftBackProject = function () { out.device_calls++; return real.apply(this, arguments); };

/* ---- ccv.DeviceBatch.backProjection ---- */
{
  const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { depth: 1, sets: job.sets.length });
  job.sets.forEach(function (f, k) { b.upload(new Uint8Array(fs.readFileSync(f)), k); });
  let threw = false;
  try { b.backProjection(0); } catch (e) { threw = true; }
  check(threw && out.device_calls === 0, 'backProjection before initTrackers must throw without reaching the addon');
  threw = false;
  b.initTrackers(new Int32Array(job.rects), 0);
  try { b.backProjection(0, 'f32'); } catch (e) { threw = e instanceof RangeError; }
  check(threw, 'an unknown kind is a RangeError');
  let last = null;
  job.expect.forEach(function (e) {
    const rgba = b.backProjection(e.set, 'rgba8'), pdf = b.backProjection(e.set, 'f64');
    check(rgba instanceof Uint8Array && rgba.length === 4 * job.n * job.w * job.h, 'set ' + e.set + ': rgba8 is a Uint8Array of 4 n w h');
    check(pdf instanceof Float64Array && pdf.length === job.n * job.w * job.h, 'set ' + e.set + ': f64 is a Float64Array of n w h');
    if (check(sameBytes(rgba, fs.readFileSync(e.rgba8)), 'set ' + e.set + ': rgba8 bytes')) out.batch_checks++;
    if (check(sameBytes(pdf, fs.readFileSync(e.f64)), 'set ' + e.set + ': f64 bytes')) out.batch_checks++;
    last = e;
  });
  /* set = -1: whatever is bound (here still the last set) */
  check(sameBytes(b.backProjection(-1), fs.readFileSync(last.rgba8)), 'set -1: the bound frames');
  /* the trackers are untouched: a track step after the back-projections equals one on a fresh batch */
  const t1 = b.trackStep(1, true);
  b.destroy();
  const b2 = new headtrackr.ccv.DeviceBatch(job.w, job.h, job.n, { depth: 1, sets: job.sets.length });
  job.sets.forEach(function (f, k) { b2.upload(new Uint8Array(fs.readFileSync(f)), k); });
  b2.initTrackers(new Int32Array(job.rects), 0);
  check(sameBytes(t1, b2.trackStep(1, true)), 'track step after back-projections == track step without');
  b2.destroy();
}

/* ---- camshift.Tracker.getBackProjectionImg ---- */
job.golden.forEach(function (g) {
  const canvasOf = function (file) { return new Canvas(g.w, g.h).setFrame(fs.readFileSync(file)); };
  const tracker = new headtrackr.camshift.Tracker({ calcAngles: g.calcAngles });
  tracker.initTracker(canvasOf(g.frames[0]), new headtrackr.camshift.Rectangle(g.rect[0], g.rect[1], g.rect[2], g.rect[3]));
  g.calls.forEach(function (f) { tracker.track(canvasOf(g.frames[f])); });
  const before = out.device_calls, sw = tracker.getSearchWindow();
  const img = tracker.getBackProjectionImg();
  check(out.device_calls === before + 1, g.name + ': getBackProjectionImg did not take the device route');
  check(img.width === g.w && img.height === g.h && img.data.length === 4 * g.w * g.h, g.name + ': ImageData shape');
  if (check(crc32(img.data) === g.crc, g.name + ': getBackProjectionImg bytes')) out.golden_checks++;
  const sw2 = tracker.getSearchWindow();
  check(sw.x === sw2.x && sw.y === sw2.y && sw.width === sw2.width && sw.height === sw2.height, g.name + ': search window untouched');
  tracker.release();
});

process.stdout.write(JSON.stringify(out) + '\n', function () { headtrackr.exitNow(out.ok ? 0 : 1); });
