'use strict';
/* The device drawImage from the JavaScript host, on a GPU (driven by tests/test_gpu_ingest.py):
 *     node tests/js/ingest_gpu.js job.json
 * job: { sw, sh, w, h, n, steps, dir (video<k>.raw: the n source frames of step k), rect, wb, wb_rect, best, best_rect, rects, tracks }
 * — expectations computed by the oracle on the expected canvases.
 *  1. ccv.drawFrames(video, canvas[, rect]) writes the bytes canvas.js's drawImage writes, through the addon's drawFramesDevice;
 *  2. ccv.DeviceBatch with opts.source: uploadSource + draw (device to device) + whitebalance / detectStep / trackStep on the drawn sets,
 *     draw with a rect, drawBound + the step functions at set = -1, and a depth-2 batch (draw waits) + detectBest.
 * Prints "ingest_gpu: ok" or the failed checks. */
const fs = require('fs');
const path = require('path');
const root = path.join(__dirname, '..', '..');
const A = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr_hip.node'));
const headtrackr = require(path.join(root, 'headtrackr_amd', 'js', 'headtrackr.js'));
const { Canvas } = require(path.join(root, 'headtrackr_amd', 'js', 'canvas.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const errors = [];
let checks = 0;
function check(cond, msg) { checks++; if (!cond && errors.length < 20) errors.push(msg); return cond; }
function same(a, b) { if (a.length !== b.length) return false; for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false; return true; }
const n = job.n, sbytes = job.sw * job.sh * 4;
const videos = [];
for (let k = 0; k < job.steps; k++) videos.push(new Uint8Array(fs.readFileSync(path.join(job.dir, 'video' + k + '.raw'))));

let deviceDraws = 0;
const realDraw = A.drawFramesDevice;
check(typeof realDraw === 'function' && typeof A.drawFrames === 'function' && typeof A.deviceDownload === 'function', 'addon exports');
A.drawFramesDevice = function () { deviceDraws++; return realDraw.apply(this, arguments); };

/* 1. ccv.drawFrames */
[null, job.rect].forEach(function (rect) {
  for (let f = 0; f < n; f++) {
    const video = new Canvas(job.sw, job.sh).setFrame(videos[0].subarray(f * sbytes, (f + 1) * sbytes));
    const host = new Canvas(job.w, job.h), dev = new Canvas(job.w, job.h);
    if (rect) host.getContext('2d').drawImage(video, rect[0], rect[1], rect[2], rect[3], 0, 0, job.w, job.h); else host.getContext('2d').drawImage(video, 0, 0, job.w, job.h);
    const before = deviceDraws;
    headtrackr.ccv.drawFrames(video, dev, rect || undefined);
    check(deviceDraws === before + 1, 'ccv.drawFrames did not take the device route');
    check(same(dev.pixels, host.pixels), 'ccv.drawFrames bytes, frame ' + f + (rect ? ' with rect' : ''));
  }
});

function bestIs(best, want, what) {
  for (let f = 0; f < n; f++) ['x', 'y', 'width', 'height', 'confidence'].forEach(function (k, i) { check(best[6 * f + i] === want[f][k], what + ': best[' + f + '].' + k + ' ' + best[6 * f + i] + ' != ' + want[f][k]); });
}
function tracksAre(t, want, what) {
  for (let f = 0; f < n; f++) {
    const g = t.subarray(9 * f, 9 * f + 9), w = want[f];
    check(Math.abs(g[0] - w.x) <= 1 && Math.abs(g[1] - w.y) <= 1 && g[2] === w.width && g[3] === w.height, what + ': track object of feed ' + f);
    let d = Math.abs(g[4] - w.angle); d = Math.min(d, Math.abs(d - Math.PI));
    check(d <= 0.5 * Math.PI / 180, what + ': angle of feed ' + f);
    check(Math.abs(g[5] - w.sw[0]) <= 1 && Math.abs(g[6] - w.sw[1]) <= 1 && g[7] === w.sw[2] && g[8] === w.sw[3], what + ': search window of feed ' + f);
  }
}

/* 2. DeviceBatch */
{
  const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 1, sets: job.steps, source: { width: job.sw, height: job.sh, sets: job.steps } });
  videos.forEach(function (v, k) { b.uploadSource(v, k); });
  for (let k = 0; k < job.steps; k++) b.draw(k, k);
  const wb = b.whitebalance(0);
  check(wb[0] === job.wb[0] && wb[1] === job.wb[1], 'whitebalance of the drawn set');
  const r = b.detectStep(0);
  bestIs(r.best, job.best, 'detectStep on the drawn set');
  check(same(r.rects, job.rects.reduce(function (a, x) { return a.concat(x); }, [])), 'initTracker rects');
  for (let k = 1; k < job.steps; k++) tracksAre(b.trackStep(k, true), job.tracks[k - 1], 'trackStep ' + k);
  /* a source rect */
  b.draw(0, 0, Int32Array.from(job.rect));
  const wr = b.whitebalance(0);
  check(wr[0] === job.wb_rect[0] && wr[1] === job.wb_rect[1], 'whitebalance of the set drawn with a rect');
  bestIs(b.detectBest(1, 1, 0).best, job.best_rect, 'detectBest on the set drawn with a rect');
  /* drawBound + set = -1 */
  b.drawBound(0);
  bestIs(b.detectStep(-1).best, job.best, 'detectStep(-1) after drawBound');
  b.drawBound(1);
  tracksAre(b.trackStep(-1, true), job.tracks[0], 'trackStep(-1) after drawBound');
  let threw = false;
  try { b.draw(0, 0, Int32Array.from([0, 0, job.sw + 1, job.sh])); } catch (e) { threw = /status -1/.test(e.message); }
  check(threw, 'a rect outside the source frame is refused with HT_ERR_INVALID');
  b.draw(0, 0);
  bestIs(b.detectBest(1, 1, 0).best, job.best, 'usable after the refused draw');
  b.destroy();
  /* depth 2: the other context reads the drawn set on its own stream, so draw waits */
  const b2 = new headtrackr.ccv.DeviceBatch(job.w, job.h, n, { depth: 2, sets: 1, source: { width: job.sw, height: job.sh, sets: 1 } });
  b2.uploadSource(videos[0], 0);
  b2.draw(0, 0);
  bestIs(b2.detectBest(4, 1, 0).best, job.best, 'depth 2: detectBest on the drawn set');
  b2.destroy();
}

process.stdout.write(errors.length ? JSON.stringify({ ok: false, checks: checks, errors: errors }) + '\n' : 'ingest_gpu: ok (' + checks + ' checks)\n', function () { headtrackr.exitNow(errors.length ? 1 : 0); });
