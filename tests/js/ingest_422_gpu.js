'use strict';
/* The packed 4:2:2 formats from the JavaScript host, on a GPU (driven by tests/test_gpu_ingest_422.py):
 *     node tests/js/ingest_422_gpu.js job.json
 * job: { sw, sh, w, h, rect, dir, rgba (the declared conversion of the content, one RGBA frame), videos: [{file (one packed frame), format,
 *        matrix, want, want_rect (expected canvases), wb}] } — the same content in both byte orders; expectations from tests/yuv422_cases.py.
 *  1. ccv.drawFrames(video, canvas[, rect]) writes the expected canvas through the addon's drawFramesYuvDevice;
 *  2. ccv.DeviceBatch with sourceFormat: uploadSource (2 B/px) + drawBound + whitebalance of the bound frames;
 *  3. ccv.DeviceBatch with mixed sources [yuyv, rgba, uyvy] holding the same picture: drawListBound, then trackers on the three canvases and
 *     cropFeeds — the patches cut from the packed feeds equal the patch cut from the RGBA feed, byte for byte, records too.
 * Prints "ingest_422_gpu: ok" or the failed checks. */
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
const read = function (name) { return new Uint8Array(fs.readFileSync(path.join(job.dir, name))); };
const fsz = 4 * ((job.sw + 1) >> 1) * job.sh;
check(A.YUV_YUYV === 4 && A.YUV_UYVY === 5, 'addon constants');
let yuvDraws = 0;
const realYuv = A.drawFramesYuvDevice;
A.drawFramesYuvDevice = function () { yuvDraws++; return realYuv.apply(this, arguments); };

const frames = {};
job.videos.forEach(function (v) {
  const data = read(v.file), want = read(v.want), wantRect = read(v.want_rect), tag = v.format + '/' + v.matrix;
  frames[v.format] = data;
  check(data.length === fsz, tag + ': a packed frame is 4 * ceil(w / 2) * h bytes');
  [null, job.rect].forEach(function (rect) {
    const dev = new Canvas(job.w, job.h), before = yuvDraws;
    headtrackr.ccv.drawFrames({ width: job.sw, height: job.sh, format: v.format, matrix: v.matrix, data: data }, dev, rect || undefined);
    check(yuvDraws === before + 1, tag + ': ccv.drawFrames took the YUV device route');
    check(same(dev.pixels, rect ? wantRect : want), tag + ': ccv.drawFrames bytes' + (rect ? ' with rect' : ''));
  });
  const b = new headtrackr.ccv.DeviceBatch(job.w, job.h, 2, { depth: 1, sets: 1, source: { width: job.sw, height: job.sh }, sourceFormat: v.format, sourceMatrix: v.matrix });
  const two = new Uint8Array(2 * fsz); two.set(data, 0); two.set(data, fsz);
  b.uploadSource(two);
  b.drawBound();
  const wb = b.whitebalance(-1);
  check(wb[0] === v.wb && wb[1] === v.wb, tag + ': whitebalance of the frames drawBound bound');
  b.destroy();
});

/* 3. mixed sources and cropFeeds */
const m = job.videos[0].matrix, rgba = read(job.rgba);
const db = new headtrackr.ccv.DeviceBatch(job.w, job.h, 3, { depth: 1, sets: 1, sources: [{ width: job.sw, height: job.sh, format: 'yuyv', matrix: m }, { width: job.sw, height: job.sh },
  { width: job.sw, height: job.sh, format: 'uyvy', matrix: m }] });
db.uploadSourceOf(0, frames.yuyv); db.uploadSourceOf(1, rgba); db.uploadSourceOf(2, frames.uyvy);
db.drawListBound(0, null);
const wl = db.whitebalance(-1);
check(wl[0] === job.videos[0].wb && wl[1] === wl[0] && wl[2] === wl[0], 'mixed sources: the three canvases hold the same picture');
const pairs = Int32Array.from([0, 0, 1, 1, 2, 2]), r = job.track;
db.initPairs(-1, pairs, Int32Array.from([].concat(r, r, r)));
db.trackPairs(-1, pairs, true);
[{ width: 24, height: 16 }, { width: 24, height: 16, prefilter: 4 }].forEach(function (o) {
  db.cropFeeds(0, Int32Array.from([0, 1, 2]), o);
  const res = db.cropResult(), pb = 24 * 16 * 4, what = 'cropFeeds' + (o.prefilter ? ' prefiltered' : '');
  const p0 = res.patches.subarray(0, pb), p1 = res.patches.subarray(pb, 2 * pb), p2 = res.patches.subarray(2 * pb, 3 * pb);
  check(same(p0, p1) && same(p2, p1), what + ': the patches from the packed feeds equal the patch from the RGBA feed');
  check(p1.some(function (x) { return x !== 0; }), what + ': the patch is not empty');
  const per = res.records.length / 3;
  for (let k = 0; k < per; k++) if (k !== 1) check(res.records[k] === res.records[per + k] && res.records[2 * per + k] === res.records[per + k], what + ': record field ' + k);  /* (field 1 is the stream) */
  check(res.records[1] === 0 && res.records[per + 1] === 1 && res.records[2 * per + 1] === 2, what + ': the records name their streams');
});
db.destroy();
process.stdout.write(errors.length ? JSON.stringify({ ok: false, checks: checks, errors: errors }) + '\n' : 'ingest_422_gpu: ok (' + checks + ' checks)\n', function () { headtrackr.exitNow(errors.length ? 1 : 0); });
